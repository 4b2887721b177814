// scene_image_demo — the host-only scene-image builder (csrc/hip/rt_scene_image.h) called through the C-ABI with no GPU and no
// context, as a program of its own so that the builder's host code can run under a sanitizer:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include \
//       tests/cpp/scene_image_demo.cpp rsoderh-raytracing_amd/csrc/hip/rsrt_api.hip rsoderh-raytracing_amd/csrc/host/*.cpp -o demo
//   ./demo tests/golden/assets/scenes/{cube,default,house,spheres_only,suzanne}.toml
// For every scene file: rsrt_scene_image_build with and without octant tables and rsrt_wide_tree_build, the image's wide-node
// section compared with the wide tree's; then hand-made trees (one node, a record in two leaves, a record in no leaf, long
// leaves) and one refusal of each kind.  Prints one line per case; exit status 0 when every call answered as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rsrt.h"
#include "rsrt_host.h"

namespace {

int failures = 0;

struct Arrays {
    std::vector<rsrt_material> materials;
    std::vector<rsrt_sphere> spheres;
    std::vector<rsrt_plane> planes;
    std::vector<rsrt_vec3> vertices, normals;
    std::vector<rsrt_triangle> triangles;
    std::vector<rsrt_primitive_info> primitives;
    std::vector<rsrt_bvh_node> nodes;
};

// the image (empty: refused, `why` has the reason) and its layout
std::vector<float> build(const Arrays &a, uint32_t flat_oriented, rsrt_scene_image_info *info, std::string *why, uint32_t n_nodes_claimed = 0)
{
    const uint32_t n_nodes = n_nodes_claimed ? n_nodes_claimed : (uint32_t)a.nodes.size();
    size_t n = 0;
    auto call = [&](float *out) {
        return rsrt_scene_image_build(a.materials.data(), (uint32_t)a.materials.size(), a.spheres.data(), (uint32_t)a.spheres.size(), a.planes.data(),
                                      (uint32_t)a.planes.size(), a.vertices.data(), (uint32_t)a.vertices.size(), a.normals.data(),
                                      (uint32_t)a.normals.size(), a.triangles.data(), (uint32_t)a.triangles.size(), a.primitives.data(),
                                      (uint32_t)a.primitives.size(), a.nodes.data(), n_nodes, flat_oriented, out, &n, info);
    };
    if (call(nullptr) != RSRT_OK) { *why = rsrt_last_error(nullptr); return {}; }
    std::vector<float> img(4 * n); // exactly the size asked for: a write past the image is a heap overflow
    if (call(img.data()) != RSRT_OK) { *why = rsrt_last_error(nullptr); return {}; }
    why->clear();
    return img;
}

void expect(bool ok, const char *what, const std::string &detail = "")
{
    std::printf("%-6s %s %s\n", ok ? "ok" : "FAILED", what, detail.c_str());
    if (!ok) failures++;
}

void whole_scene(const char *path, const Arrays &a)
{
    rsrt_scene_image_info info, plain;
    std::string why;
    const std::vector<float> img = build(a, 1, &info, &why), img0 = build(a, 0, &plain, &why);
    expect(!img.empty() && !img0.empty() && img.size() == 4 * info.n_float4 && img0.size() + 4 * 8 * (size_t)info.flat_ostride == img.size(), path, why);
    uint32_t n_w = 0;
    const rsrt_status st = rsrt_wide_tree_build(a.primitives.data(), (uint32_t)a.primitives.size(), a.nodes.data(), (uint32_t)a.nodes.size(), nullptr, &n_w, nullptr);
    bool same = (st == RSRT_OK) == (info.wide_ok != 0) && n_w == info.n_wnodes;
    if (same && st == RSRT_OK) {
        std::vector<float> wn(32 * (size_t)n_w);
        std::vector<uint32_t> old_of_new(a.primitives.size());
        same = rsrt_wide_tree_build(a.primitives.data(), (uint32_t)a.primitives.size(), a.nodes.data(), (uint32_t)a.nodes.size(), wn.data(), &n_w, old_of_new.data()) == RSRT_OK &&
               std::memcmp(wn.data(), img.data() + 4 * info.wnodes, wn.size() * sizeof(float)) == 0;
    }
    expect(same, "  wide tree == the image's wnodes section");
}

void refusal(const char *want, const Arrays &a, uint32_t n_nodes_claimed = 0)
{
    rsrt_scene_image_info info;
    std::string why;
    const bool refused = build(a, 1, &info, &why, n_nodes_claimed).empty();
    expect(refused && why.find(want) != std::string::npos, want, refused ? "" : "(not refused)");
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: scene_image_demo scene.toml [scene.toml ...]\n"); return 2; }
    Arrays first;
    for (int k = 1; k < argc; k++) {
        char err[2048] = {0};
        rsrt_scene *scene = nullptr;
        if (rsrt_scene_load_toml(argv[k], &scene, err, sizeof err) != 0) { std::fprintf(stderr, "%s\n", err); return 1; }
        rsrt_scene_counts c;
        rsrt_scene_get_counts(scene, &c);
        Arrays a;
        a.materials.assign(rsrt_scene_materials(scene), rsrt_scene_materials(scene) + c.n_materials);
        a.spheres.assign(rsrt_scene_spheres(scene), rsrt_scene_spheres(scene) + c.n_spheres);
        a.planes.assign(rsrt_scene_planes(scene), rsrt_scene_planes(scene) + c.n_planes);
        a.vertices.assign(rsrt_scene_vertices(scene), rsrt_scene_vertices(scene) + c.n_vertices);
        a.normals.assign(rsrt_scene_normals(scene), rsrt_scene_normals(scene) + c.n_normals);
        a.triangles.assign(rsrt_scene_triangles(scene), rsrt_scene_triangles(scene) + c.n_triangles);
        a.primitives.assign(rsrt_scene_primitives(scene), rsrt_scene_primitives(scene) + c.n_primitives);
        a.nodes.assign(rsrt_scene_bvh_nodes(scene), rsrt_scene_bvh_nodes(scene) + c.n_bvh_nodes);
        rsrt_scene_free(scene);
        whole_scene(argv[k], a);
        if (k == 1) first = a;
    }
    // ---- hand-made trees over the first scene's arrays
    const Arrays &s = first;
    if (s.nodes.size() < 3 || s.primitives.size() < 3 || s.triangles.empty() || s.materials.empty()) { std::fprintf(stderr, "the first scene is too small for the hand-made cases\n"); return 2; }
    rsrt_scene_image_info info;
    std::string why;
    const uint32_t n_p = (uint32_t)s.primitives.size();
    {
        Arrays a = s; // one node: a leaf with every record
        a.nodes.resize(1);
        a.nodes[0].primitives_or_second_child_index = 0;
        a.nodes[0].primitives_len = n_p;
        expect(!build(a, 1, &info, &why).empty() && info.n_leaves == 1 && !info.wide_ok && info.typed_leaves == (n_p <= 8), "one-node tree", why);
    }
    auto three = [&](uint32_t first_a, uint32_t len_a, uint32_t first_b, uint32_t len_b) { // a root and two leaves, all with the root's box
        Arrays a = s;
        a.nodes.assign(3, s.nodes[0]);
        a.nodes[0].primitives_or_second_child_index = 2; a.nodes[0].primitives_len = 0; a.nodes[0].split_axis = 0;
        a.nodes[1].primitives_or_second_child_index = first_a; a.nodes[1].primitives_len = len_a;
        a.nodes[2].primitives_or_second_child_index = first_b; a.nodes[2].primitives_len = len_b;
        return a;
    };
    {
        Arrays a = three(0, 2, 1, 2); // record 1 in both leaves
        a.primitives.resize(3);
        expect(!build(a, 1, &info, &why).empty() && !info.flat_ok && !info.wide_ok, "a record in two leaves", why);
    }
    expect(!build(three(0, 1, 2, n_p - 2), 1, &info, &why).empty() && !info.wide_ok, "a record in no leaf", why);
    expect(!build(three(0, n_p / 2, n_p / 2, n_p - n_p / 2), 1, &info, &why).empty() && info.typed_leaves == (n_p - n_p / 2 <= 8), "two long leaves", why);
    // ---- one refusal of each kind
    { Arrays a = s; a.triangles[0].material_id = (uint32_t)s.materials.size(); refusal("triangle 0: material_id", a); }
    { Arrays a = s; a.triangles[0].vertex_2 = (uint32_t)s.vertices.size(); refusal("triangle 0: vertex index out of range", a); }
    { Arrays a = s; a.triangles[0].normal_0 = (uint32_t)s.normals.size(); refusal("triangle 0: normal index out of range", a); }
    { Arrays a = s; a.primitives[1].index = 1u << 20; refusal("primitive 1: type", a); }
    { Arrays a = s; a.nodes[0].primitives_or_second_child_index = (uint32_t)s.nodes.size(); refusal("bvh interior node 0: bad child index / axis", a); }
    { Arrays a = three(0, 1, 1, n_p); refusal("bvh leaf 2: primitive range out of bounds", a); }
    {
        Arrays a = s; // 0 -> (1, 2), 1 -> (2, 3): node 2 is the second child of 0 and the first of 1
        a.nodes.assign(4, s.nodes[0]);
        const uint32_t link[4] = {2, 3, 0, 1}, len[4] = {0, 0, 1, 1};
        for (int i = 0; i < 4; i++) { a.nodes[i].primitives_or_second_child_index = link[i]; a.nodes[i].primitives_len = len[i]; a.nodes[i].split_axis = 0; }
        refusal("bvh node 2 reachable twice", a);
        const uint32_t link2[4] = {3, 0, 1, 2}, len2[4] = {0, 1, 1, 1}; // 0 -> (1, 3): nobody names node 2
        for (int i = 0; i < 4; i++) { a.nodes[i].primitives_or_second_child_index = link2[i]; a.nodes[i].primitives_len = len2[i]; }
        refusal("bvh node 2 is not reachable from the root", a);
        uint32_t n_w = 0;
        expect(rsrt_wide_tree_build(a.primitives.data(), n_p, a.nodes.data(), 4, nullptr, &n_w, nullptr) != RSRT_OK, "the wide-tree entry point refuses that tree too");
    }
    refusal("nodes exceed the 25-bit traversal cursor", s, 0x1ffffffu); // (refused by the count alone: the array is not read)
    { Arrays a = s; a.nodes.clear(); refusal("bvh_nodes is empty", a); }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
