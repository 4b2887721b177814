// rt_scene_image.h — the scene's device image, built on the host: validate_scene checks the caller's arrays, build_scene_image lays
// every table the traversals read out in one float4 array and says where each lies (rsrt_scene_image_info, include/rsrt.h).
// Plain C++17: no HIP runtime call, no context — rsrt_upload_scene copies the image to the device and fills DevScene as
// blob + offset; rsrt_scene_image_build and rsrt_wide_tree_build hand the same results to CPU tests (tests/test_scene_image.py).
// rsrt_api.hip includes this after the device headers whose constants it needs (rt_device.h: PRIM_*, RT_END, RT_WSTACK, RT_WSPILL;
// rt_coop.h: RT_COOP_MAX_RECORDS, RT_COOP_MAX_NODES).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace {

static_assert(sizeof(rsrt_scene_image_info) == 14 * 8 + 84 * 4, "rsrt_scene_image_info has no padding: tests hash its bytes");

inline float fmaxh(float a, float b) { return a < b ? b : a; }
inline float fminh(float a, float b) { return b < a ? b : a; }
inline float saturateh(float x) { return fminh(fmaxh(x, 0.0f), 1.0f); }
inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// record of one primitive (4 float4), see rt_device.h
void make_sphere_record(const rsrt_sphere &s, float4 *r)
{
    r[0] = f4(s.pos[0], s.pos[1], s.pos[2], u2f(PRIM_SPHERE | (s.material_id << 2)));
    r[1] = f4(s.radius, s.radius * s.radius, 0, 0);
    r[2] = r[3] = f4(0, 0, 0, 0);
}
void make_plane_record(const rsrt_plane &p, float4 *r)
{
    r[0] = f4(p.pos[0], p.pos[1], p.pos[2], u2f(PRIM_PLANE | (p.material_id << 2)));
    r[1] = f4(p.normal[0], p.normal[1], p.normal[2], 0);
    r[2] = f4(p.base_change_matrix[0][0], p.base_change_matrix[1][0], p.base_change_matrix[2][0], 0); // row x
    r[3] = f4(p.base_change_matrix[0][2], p.base_change_matrix[1][2], p.base_change_matrix[2][2], 0); // row z
}
void make_triangle_record(const rsrt_triangle &t, uint32_t index, const rsrt_vec3 *v, float4 *r)
{
    const float *a = v[t.vertex_0].v, *b = v[t.vertex_1].v, *c = v[t.vertex_2].v;
    r[0] = f4(a[0], a[1], a[2], u2f(PRIM_TRIANGLE | (t.material_id << 2)));
    r[1] = f4(b[0] - a[0], b[1] - a[1], b[2] - a[2], u2f(index)); // edge_0, shader.wgsl:415
    r[2] = f4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0);          // edge_1, :416
    r[3] = f4(0, 0, 0, 0);
}
// Do two primitive records put the same numbers into their intersection test (type and geometry words; not the material, not a
// triangle's normal index)?  Then every ray gets the same t from both.
bool same_test(const float4 *a, const float4 *b)
{
    uint32_t ta, tb;
    memcpy(&ta, &a[0].w, 4); memcpy(&tb, &b[0].w, 4);
    if ((ta & 3u) != (tb & 3u) || memcmp(&a[0], &b[0], 12) != 0) return false;
    if ((ta & 3u) == PRIM_TRIANGLE) return memcmp(&a[1], &b[1], 12) == 0 && memcmp(&a[2], &b[2], 12) == 0;
    return memcmp(a + 1, b + 1, 3 * sizeof(float4)) == 0;
}
// make_bsdf_material / surface_f0 / surface_kd / lobe probabilities (shader.wgsl:850-881, :1147-1148)
void make_material_record(const rsrt_material &m, float4 *r)
{
    const float t = saturateh(m.metallic);
    float f0[3], kd[3];
    for (int k = 0; k < 3; k++) f0[k] = (1.0f - t) * 0.04f + t * m.color[k];
    const float maxf0 = fmaxh(f0[0], fmaxh(f0[1], f0[2]));
    for (int k = 0; k < 3; k++) kd[k] = (m.color[k] * (1.0f - t)) * (1.0f - maxf0);
    const float alpha = fmaxh(0.001f, m.roughness * m.roughness);
    const float ps = saturateh(0.2126f * f0[0] + 0.7152f * f0[1] + 0.0722f * f0[2]);
    r[0] = f4(m.color[0], m.color[1], m.color[2], m.metallic);
    r[1] = f4(f0[0], f0[1], f0[2], alpha);
    r[2] = f4(m.emission[0], m.emission[1], m.emission[2], ps);
    r[3] = f4(kd[0], kd[1], kd[2], 1.0f - ps);
}

// ---- what the builders below ask of a tree (all of them after validate_tree: every index they follow is in bounds)
inline uint32_t second_child(const rsrt_bvh_node &nd) { return nd.primitives_or_second_child_index; } // of an interior node; its first child follows it
inline uint32_t first_record(const rsrt_bvh_node &nd) { return nd.primitives_or_second_child_index; } // of a leaf

// a node's box surface area (halved; 0 for a box with a NaN): a ray meets a node about as often as its box is large
double box_area(const rsrt_bvh_node &nd)
{
    const double dx = (double)nd.bounds_max[0] - nd.bounds_min[0], dy = (double)nd.bounds_max[1] - nd.bounds_min[1],
                 dz = (double)nd.bounds_max[2] - nd.bounds_min[2];
    const double a = dx * dy + dy * dz + dz * dx;
    return a == a ? a : 0.0;
}

// Every child box lies inside its parent's, and no two leaves name the same record: what makes skipping binary nodes exact (the
// wide walks) and gives every record ONE position in a visiting order (the flat loop's rank bytes).
bool boxes_nest_and_leaves_share_no_record(const rsrt_bvh_node *nodes, uint32_t n_nodes, uint32_t n_prims)
{
    std::vector<uint8_t> covered(n_prims, 0);
    for (uint32_t i = 0; i < n_nodes; i++) {
        const rsrt_bvh_node &nd = nodes[i];
        for (uint32_t k = 0; k < nd.primitives_len; k++) {
            uint8_t &c = covered[first_record(nd) + k];
            if (c) return false;
            c = 1;
        }
        if (nd.primitives_len == 0)
            for (uint32_t c : {i + 1u, second_child(nd)})
                for (int k = 0; k < 3; k++)
                    if (!(nodes[c].bounds_min[k] >= nd.bounds_min[k] && nodes[c].bounds_max[k] <= nd.bounds_max[k])) return false;
    }
    return true;
}

// The reference's near-child-first walk for ray-sign octant q (bit 0 x, bit 1 y, bit 2 z), every box "hit": visit(node, escape) in
// visiting order, escape = the node the walk goes to when this node's subtree is done (RT_END: nowhere).
template <class Visit>
void walk_octant(const rsrt_bvh_node *nodes, uint32_t q, Visit visit)
{
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, RT_END}}; // node, its escape
    while (!st.empty()) {
        auto [i, esc] = st.back();
        st.pop_back();
        visit(i, esc);
        const rsrt_bvh_node &nd = nodes[i];
        if (nd.primitives_len != 0) continue;
        const bool far_first = (q >> nd.split_axis) & 1u; // sign(inv_dir[axis]) < 0: second child is nearer
        const uint32_t near_c = far_first ? second_child(nd) : i + 1, far_c = far_first ? i + 1 : second_child(nd);
        st.push_back({far_c, esc}); // far child: visited after the near one
        st.push_back({near_c, far_c});
    }
}

// ---- wide walk (rt_device.h, trace_wide): the binary tree collapsed into 4-wide nodes, laid out hottest-first (build_wide_tree)
struct WideNode { uint32_t ch[4]; uint32_t n_ch, n_int, first_child; }; // binary nodes of the children (interior ones first), index of the first interior child's wide node
// false: the scene does not qualify — the walk needs nested boxes and leaves that share no record, leaves of <= 8 records that
// cover every record (whole leaves are moved: the permutation must be total) and a wide tree of at most RT_WSTACK + RT_WSPILL + 1
// levels (the walk's stack: eight registers and sixteen overflow words).  prims_out / nodes_out: `prims` with whole leaves
// reordered so that the records of a wide node's leaf children are contiguous, and `nodes` with the leaves' first indices pointing
// there; old_of_new (may be NULL): for every new record index the old one.
bool build_wide_tree(const rsrt_bvh_node *nodes, uint32_t n_nodes, const rsrt_primitive_info *prims, uint32_t n_prims, std::vector<WideNode> &wide,
                     std::vector<rsrt_primitive_info> &prims_out, std::vector<rsrt_bvh_node> &nodes_out, std::vector<uint32_t> *old_of_new, uint32_t *wide_depth = nullptr)
{
    wide.clear();
    if (n_nodes < 3 || nodes[0].primitives_len != 0) return false;
    uint64_t in_leaves = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (nodes[i].primitives_len > 8) return false;
        in_leaves += nodes[i].primitives_len;
    }
    if (in_leaves != n_prims || !boxes_nest_and_leaves_share_no_record(nodes, n_nodes, n_prims)) return false; // (as many as there are, none twice: all covered)
    // Array order = the order in which nodes are ALLOCATED, and a node's interior children are allocated together, when the node is
    // expanded (child k = first child + k).  Nodes are expanded largest box first (a ray meets a node about as often as its box is large, and
    // a child's box lies inside its parent's), so that the array's head — the part the kernel stages in LDS — is the part of the tree the
    // rays visit most.  (Breadth-first instead, the first version: 0-1.5 % slower, profiles/r03_walk_bounds.txt.)
    std::vector<uint32_t> queue{0u}, level{0u}; // binary roots of the wide nodes, in array order
    uint32_t wdepth = 1;
    using Pending = std::pair<double, uint32_t>; // (box area, array index) of a node still to expand
    const auto expand_later = [](const Pending &a, const Pending &b) { return a.first < b.first || (a.first == b.first && a.second > b.second); };
    std::vector<Pending> heap{{box_area(nodes[0]), 0u}};
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), expand_later);
        const size_t qi = heap.back().second;
        heap.pop_back();
        const uint32_t r = queue[qi];
        std::vector<uint32_t> ch{r + 1u, second_child(nodes[r])};
        while (ch.size() < 4) { // open the interior child with the largest box
            int best = -1;
            for (size_t k = 0; k < ch.size(); k++)
                if (nodes[ch[k]].primitives_len == 0 && (best < 0 || box_area(nodes[ch[k]]) > box_area(nodes[ch[best]]))) best = (int)k;
            if (best < 0) break;
            const uint32_t c = ch[best];
            ch[best] = c + 1u;
            ch.insert(ch.begin() + best + 1, second_child(nodes[c]));
        }
        WideNode w{};
        for (uint32_t c : ch) if (nodes[c].primitives_len == 0) w.ch[w.n_ch++] = c; // interior children first ...
        w.n_int = w.n_ch;
        for (uint32_t c : ch) if (nodes[c].primitives_len != 0) w.ch[w.n_ch++] = c; // ... then the leaves
        w.first_child = (uint32_t)queue.size(); // consecutive: allocated here and now
        for (uint32_t k = 0; k < w.n_int; k++) {
            heap.push_back({box_area(nodes[w.ch[k]]), (uint32_t)queue.size()});
            std::push_heap(heap.begin(), heap.end(), expand_later);
            queue.push_back(w.ch[k]);
            level.push_back(level[qi] + 1u);
            wdepth = std::max(wdepth, level[qi] + 2u);
        }
        if (wide.size() < queue.size()) wide.resize(queue.size());
        wide[qi] = w;
    }
    wide.resize(queue.size());
    if (wdepth > RT_WSTACK + RT_WSPILL + 1u || wide.size() >= (1u << 27)) { wide.clear(); return false; } // (deeper than the walk's stack: registers + overflow columns)
    if (wide_depth) *wide_depth = wdepth;
    // whole leaves, in the order the wide nodes list them
    prims_out.resize(n_prims);
    nodes_out.assign(nodes, nodes + n_nodes);
    if (old_of_new) old_of_new->resize(n_prims);
    uint32_t at = 0;
    for (const WideNode &w : wide)
        for (uint32_t k = w.n_int; k < w.n_ch; k++) {
            const rsrt_bvh_node &lf = nodes[w.ch[k]];
            for (uint32_t j = 0; j < lf.primitives_len; j++) {
                prims_out[at + j] = prims[first_record(lf) + j];
                if (old_of_new) (*old_of_new)[at + j] = first_record(lf) + j;
            }
            nodes_out[w.ch[k]].primitives_or_second_child_index = at;
            at += lf.primitives_len;
        }
    return true;
}
// the device records of the wide nodes (8 float4 each; rt_device.h, DevScene::wnodes) from the PERMUTED nodes / primitives
void fill_wide_nodes(const std::vector<WideNode> &wide, const rsrt_bvh_node *nodes, const rsrt_primitive_info *prims, float4 *out)
{
    for (size_t wi = 0; wi < wide.size(); wi++) {
        const WideNode &w = wide[wi];
        float4 *q = out + 8 * wi;
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // see DevScene::wnodes
        words[0] = w.first_child | (((1u << w.n_int) - 1u) << 26);
        if (w.n_ch > w.n_int) words[1] = first_record(nodes[w.ch[w.n_int]]); // the leaves' records are contiguous from here
        for (uint32_t k = 0; k < 4; k++) {
            if (k >= w.n_ch) { q[2 * k] = q[2 * k + 1] = f4(0, 0, 0, 0); continue; } // (an empty slot's box may "hit": no mask names it)
            const rsrt_bvh_node &nd = nodes[w.ch[k]]; // the child's EXACT box
            q[2 * k] = f4(nd.bounds_min[0], nd.bounds_min[1], nd.bounds_min[2], 0);
            q[2 * k + 1] = f4(nd.bounds_max[0], nd.bounds_max[1], nd.bounds_max[2], 0);
            if (k < w.n_int) continue;
            const uint32_t off = first_record(nd) - words[1]; // < 32: four leaves of at most eight records
            words[4 + k] = ((1u << nd.primitives_len) - 1u) << off;
            for (uint32_t j = 0; j < nd.primitives_len; j++) {
                const uint32_t ty = prims[first_record(nd) + j].primitive_type;
                if (ty >= 2) words[2] |= 1u << (off + j);
                else if (ty == 1) words[3] |= 1u << (off + j);
            }
        }
        for (int k = 0; k < 8; k++) q[k].w = u2f(words[k]);
    }
}

// ---- the caller's arrays
std::string message(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// The arrays of rsrt_upload_scene (include/rsrt.h), in its order.
struct SceneInputs {
    const rsrt_material *materials; uint32_t n_materials; const rsrt_sphere *spheres; uint32_t n_spheres;
    const rsrt_plane *planes; uint32_t n_planes; const rsrt_vec3 *vertices; uint32_t n_vertices;
    const rsrt_vec3 *normals; uint32_t n_normals; const rsrt_triangle *triangles; uint32_t n_triangles;
    const rsrt_primitive_info *primitives; uint32_t n_primitives; const rsrt_bvh_node *nodes; uint32_t n_nodes;
};

// tree shape: pre-order layout (children after their parent) => traversal terminates; every node reached exactly once, every leaf's
// records within the primitive array.  "" and the depth, or why the tree is refused.
std::string validate_tree(const rsrt_bvh_node *nodes, uint32_t n_nodes, uint32_t n_primitives, uint32_t *depth_out)
{
    uint32_t depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}}; // node, depth
    std::vector<uint8_t> seen(n_nodes, 0);
    while (!st.empty()) {
        auto [i, d] = st.back();
        st.pop_back();
        if (seen[i]) return message("bvh node %u reachable twice", i);
        seen[i] = 1;
        depth = std::max(depth, d);
        const rsrt_bvh_node &nd = nodes[i];
        if (nd.primitives_len > 0) {
            if (nd.primitives_len > 0xffffu || (uint64_t)first_record(nd) + nd.primitives_len > n_primitives)
                return message("bvh leaf %u: primitive range out of bounds", i);
        } else {
            const uint32_t second = second_child(nd);
            if (nd.split_axis > 2 || i + 1 >= n_nodes || second <= i + 1 || second >= n_nodes)
                return message("bvh interior node %u: bad child index / axis", i);
            st.push_back({second, d + 1});
            st.push_back({i + 1, d + 1});
        }
    }
    for (uint32_t i = 0; i < n_nodes; i++) // (the tables of build_scene_image are indexed by every node)
        if (!seen[i]) return message("bvh node %u is not reachable from the root", i);
    *depth_out = depth;
    return "";
}

// Every index the kernels will follow, and the tree's shape.  "" and the tree's depth, or why the scene is refused.
std::string validate_scene(const SceneInputs &in, uint32_t *depth_out)
{
    if (in.n_nodes == 0 || !in.nodes) return "bvh_nodes is empty";
    if (in.n_nodes >= RT_END) return message("bvh_nodes: %u nodes exceed the 25-bit traversal cursor", in.n_nodes);
    if ((in.n_materials && !in.materials) || (in.n_spheres && !in.spheres) || (in.n_planes && !in.planes) || (in.n_vertices && !in.vertices) ||
        (in.n_normals && !in.normals) || (in.n_triangles && !in.triangles) || (in.n_primitives && !in.primitives))
        return "a non-empty array has a NULL pointer";
    if (in.n_materials >= (1u << 30)) return "too many materials";
    for (uint32_t i = 0; i < in.n_spheres; i++)
        if (in.spheres[i].material_id >= in.n_materials) return message("sphere %u: material_id %u out of range", i, in.spheres[i].material_id);
    for (uint32_t i = 0; i < in.n_planes; i++)
        if (in.planes[i].material_id >= in.n_materials) return message("plane %u: material_id %u out of range", i, in.planes[i].material_id);
    for (uint32_t i = 0; i < in.n_triangles; i++) {
        const rsrt_triangle &t = in.triangles[i];
        if (t.material_id >= in.n_materials) return message("triangle %u: material_id %u out of range", i, t.material_id);
        if (t.vertex_0 >= in.n_vertices || t.vertex_1 >= in.n_vertices || t.vertex_2 >= in.n_vertices)
            return message("triangle %u: vertex index out of range", i);
        if (t.normal_0 >= in.n_normals || t.normal_1 >= in.n_normals || t.normal_2 >= in.n_normals)
            return message("triangle %u: normal index out of range", i);
    }
    for (uint32_t i = 0; i < in.n_primitives; i++) {
        const rsrt_primitive_info &p = in.primitives[i];
        const uint32_t lim = p.primitive_type == 0 ? in.n_spheres : (p.primitive_type == 1 ? in.n_planes : (p.primitive_type == 2 ? in.n_triangles : 0));
        if (p.index >= lim) return message("primitive %u: type %u index %u out of range", i, p.primitive_type, p.index);
    }
    return validate_tree(in.nodes, in.n_nodes, in.n_primitives, depth_out);
}

// ---- fixed-order traversal (rt_device.h, trace_preorder): the walk's node array ("pnodes").  Every interior node carries BOTH its
// links explicitly — where to go when its box is hit (its first child) and when it is missed (the pre-order successor of its
// subtree) — and a leaf is followed by its successor, so the array may be laid out in any order.  It is laid out in two levels:
// first a TOP BLOCK, the nodes a ray is most likely to meet (greedy by box surface area from the root: a child's box lies inside
// its parent's, so the set is closed under "parent of"), in their pre-order; then everything else, in pre-order.  The kernel keeps
// the top block in LDS (one copy per CU) and reads the rest from global memory: on the 15,488-triangle grid scene 1,400 of 8,731
// nodes take ~80 % of the box tests.  Where a leaf's successor is not the next array element (a subtree leaves or re-enters the top
// block) a JUMP element is inserted: an interior-type record whose two links are equal and whose box is never tested.
struct PNode { uint32_t old; uint32_t jump_to; }; // old == UINT32_MAX: a jump element to old node `jump_to` (n_nodes = end)
struct PNodeList {
    std::vector<PNode> elems;
    std::vector<uint32_t> succ; // pre-order successor of old node i's subtree (n_nodes = end)
    uint32_t top_elems = 0;     // elements of the top block, jump elements included: at most top_max unless one node alone needs more
};
PNodeList build_pnode_list(const rsrt_bvh_node *nodes, uint32_t n_nodes, uint32_t top_max)
{
    PNodeList out;
    out.succ.assign(n_nodes, n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) // (a parent comes before its children)
        if (nodes[i].primitives_len == 0) {
            out.succ[i + 1] = second_child(nodes[i]); // the first child's subtree ends where the second child begins
            out.succ[second_child(nodes[i])] = out.succ[i];
        }
    for (uint32_t want = std::min<uint32_t>(n_nodes, top_max);; want = want * 7 / 8) {
        std::vector<uint8_t> in_top(n_nodes, 0);
        std::vector<std::pair<double, uint32_t>> heap{{box_area(nodes[0]), 0u}}; // greedy by surface area
        for (uint32_t taken = 0; !heap.empty() && taken < want; taken++) {
            std::pop_heap(heap.begin(), heap.end());
            const uint32_t i = heap.back().second;
            heap.pop_back();
            in_top[i] = 1;
            if (nodes[i].primitives_len == 0)
                for (uint32_t c : {i + 1u, second_child(nodes[i])}) {
                    heap.push_back({box_area(nodes[c]), c});
                    std::push_heap(heap.begin(), heap.end());
                }
        }
        out.elems.clear();
        for (int pass = 0; pass < 2; pass++) { // top block, then the rest; both in pre-order (= index order)
            std::vector<uint32_t> order;
            for (uint32_t i = 0; i < n_nodes; i++)
                if ((in_top[i] != 0) == (pass == 0)) order.push_back(i);
            for (size_t k = 0; k < order.size(); k++) {
                const uint32_t i = order[k];
                out.elems.push_back({i, 0u});
                const uint32_t follows = k + 1 < order.size() ? order[k + 1] : 0xffffffffu; // (the rest's first element never follows the top block's last)
                if (nodes[i].primitives_len != 0 && out.succ[i] != follows) out.elems.push_back({0xffffffffu, out.succ[i]});
            }
            if (pass == 0) out.top_elems = (uint32_t)out.elems.size();
        }
        if (out.top_elems <= top_max || want <= 1) return out;
    }
}

// ---- the flat loop's two-level cull (rt_device.h, RT_FLAT_CULL): the interior nodes two levels below the root, each with the leaves
// under it as a mask; the leaves above that level are always tested.  leaf_index: a leaf node's number in the leaf list.
void fill_cull_groups(const rsrt_bvh_node *nodes, const std::vector<uint32_t> &leaf_index, rsrt_scene_image_info &info)
{
    const uint32_t cull_depth = 2u; // (1 / 2 / 3 below the root measured alike, profiles/r03_fusion_ab.txt)
    std::vector<uint32_t> under(leaf_index.size()); // the leaves under a node, as a mask (children come after their parent)
    for (uint32_t i = (uint32_t)under.size(); i-- > 0;)
        under[i] = nodes[i].primitives_len != 0 ? 1u << leaf_index[i] : under[i + 1] | under[second_child(nodes[i])];
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}}; // node, depth
    info.cull_always = 0u;
    while (!st.empty()) {
        auto [i, d] = st.back();
        st.pop_back();
        const rsrt_bvh_node &nd = nodes[i];
        if (nd.primitives_len != 0) { info.cull_always |= under[i]; continue; }
        if (d == cull_depth && info.n_cull < 8) {
            for (int k = 0; k < 3; k++) { info.cull_min[info.n_cull][k] = nd.bounds_min[k]; info.cull_max[info.n_cull][k] = nd.bounds_max[k]; }
            info.cull_mask[info.n_cull++] = under[i];
            continue;
        }
        st.push_back({i + 1, d + 1});
        st.push_back({second_child(nd), d + 1});
    }
}

// ---- the image
struct SceneImage {
    std::vector<float4> image;
    rsrt_scene_image_info info;
    std::string error; // not empty: the scene is refused, image and info mean nothing
};

// The image of a scene validate_scene has passed (depth: what it returned):
//   nodes | escape links | prims | tri normals | materials | fallback spheres | fallback planes | flat leaves [| their octant tables]
// — as far as that the LDS image of a small scene — then flat ranks | pre-order nodes | record ranks | wide nodes.
// flat_oriented: the flat loop may have its octant tables (where they fit); small_image_bytes: the largest image that goes to LDS
// whole; hybrid_room_f4: the LDS room of a mid-size scene's walk, which bounds the pre-order nodes' top block.
SceneImage build_scene_image(const SceneInputs &in, uint32_t depth, bool flat_oriented, size_t small_image_bytes, uint32_t hybrid_room_f4)
{
    SceneImage out;
    rsrt_scene_image_info &info = out.info;
    memset(&info, 0, sizeof info);
    const uint32_t n_nodes = in.n_nodes, n_prims = in.n_primitives;
    // ---- wide walk: whole leaves are moved so that the records of a wide node's leaf children are contiguous.  `prims` and the
    // leaves' first indices are re-pointed at the permuted copies and everything below is built from those: a record's index is
    // internal to the device image, ties are decided by the visiting ranks computed from the tree.
    const rsrt_primitive_info *prims = in.primitives;
    const rsrt_bvh_node *nodes = in.nodes;
    std::vector<WideNode> wide;
    std::vector<rsrt_primitive_info> prims_perm;
    std::vector<rsrt_bvh_node> nodes_perm;
    uint32_t wide_depth = 0;
    const bool wide_ok = build_wide_tree(nodes, n_nodes, prims, n_prims, wide, prims_perm, nodes_perm, nullptr, &wide_depth);
    if (wide_ok) {
        prims = prims_perm.data();
        nodes = nodes_perm.data();
    }
    // ---- one near-child-first walk per octant gives the threaded traversal its links, escape[octant][node] (trace_threaded), and
    // every record its visiting rank, prim_rank[octant][record] (trace_preorder): the position at which the reference's walk meets
    // it, which decides equal t whatever order the records are really tested in.  A record that several leaves share keeps the rank
    // of its FIRST visit (the reference's strict < keeps the first of equals); one that no leaf names keeps 0xffffffff.
    std::vector<uint32_t> escape(8ull * n_nodes, RT_END), prim_rank(8ull * n_prims, 0xffffffffu);
    for (uint32_t q = 0; q < 8; q++) {
        uint32_t pos = 0;
        walk_octant(nodes, q, [&](uint32_t i, uint32_t esc) {
            escape[(size_t)q * n_nodes + i] = esc;
            for (uint32_t k = 0; k < nodes[i].primitives_len; k++, pos++) {
                uint32_t &rk = prim_rank[(size_t)q * n_prims + first_record(nodes[i]) + k];
                rk = std::min(rk, pos);
            }
        });
    }
    // ---- flat small-scene traversal (trace_flat): at most 64 records of each kind (a hit is carried as a 6-bit record index + 2-bit
    // source in the idle cursor bits), few enough leaves that testing every leaf box beats the tree walk, nested boxes and leaves
    // that share no record: its rank table, the ranks above as bytes (0 for a record no leaf names), gives every record ONE position
    std::vector<uint32_t> leaf_nodes, leaf_index(n_nodes, 0u);
    bool typed_leaves = true; // no leaf has more than 8 records: the leaf nodes' words carry per-type masks
    for (uint32_t i = 0; i < n_nodes; i++)
        if (nodes[i].primitives_len != 0) {
            leaf_index[i] = (uint32_t)leaf_nodes.size();
            leaf_nodes.push_back(i);
            typed_leaves = typed_leaves && nodes[i].primitives_len <= 8;
        }
    const bool flat_ok = n_prims <= 64 && in.n_spheres <= 64 && in.n_planes <= 64 && leaf_nodes.size() <= 32 &&
                         boxes_nest_and_leaves_share_no_record(nodes, n_nodes, n_prims);
    uint32_t flat_rank[8 * 16] = {};
    uint64_t tri_mask = 0, plane_mask = 0;
    if (flat_ok)
        for (uint32_t p = 0; p < n_prims; p++) {
            if (prims[p].primitive_type >= 2) tri_mask |= 1ull << p;
            else if (prims[p].primitive_type == 1) plane_mask |= 1ull << p;
            for (uint32_t q = 0; q < 8; q++)
                if (prim_rank[q * n_prims + p] != 0xffffffffu) flat_rank[q * 16 + (p >> 2)] |= prim_rank[q * n_prims + p] << (8 * (p & 3));
        }
    const PNodeList pl = build_pnode_list(nodes, n_nodes, hybrid_room_f4 / 2u); // (top-block elements that fit beside sixteen path pools, 32 B each)
    const uint32_t n_pnodes = (uint32_t)pl.elems.size();
    if (n_pnodes >= RT_END) { out.error = message("bvh_nodes: %u traversal elements exceed the 25-bit cursor", n_pnodes); return out; }
    // The leaf boxes once more for each ray-sign octant q (as trace_flat computes it), corners in slab order: {near.xyz, mask lo}
    // {far.xyz, mask hi}, near = the max corner on the axes whose bit is set.  Tables are 2 x an odd number of float4s apart, so the
    // eight octants' copies of one leaf lie in eight different 16-byte cells of LDS's 256-byte bank row (a ds_read_b128 of a wave of
    // mixed octants has no bank conflict).  Only where the image with them still fits beside the path pools: a scene they would push
    // out of LDS keeps the loop that orders the values itself.
    const size_t ostride_f4 = 2 * (leaf_nodes.size() | 1);
    // ---- the layout
    info.nodes = 0;
    info.escape = info.nodes + 2ull * n_nodes;
    info.prims = info.traversal_head_f4 = info.escape + (8ull * n_nodes + 3) / 4; // nodes | escape links: what the hybrid view keeps in LDS
    info.tri_normals = info.prims + 4ull * n_prims;
    info.materials = info.tri_normals + 3ull * in.n_triangles;
    info.fb_spheres = info.materials + 4ull * in.n_materials;
    info.fb_planes = info.fb_spheres + 4ull * in.n_spheres;
    info.flat_leaves = info.fb_planes + 4ull * in.n_planes;
    uint64_t lds_f4 = info.flat_leaves + (flat_ok ? 2 * leaf_nodes.size() : 0);
    if (flat_ok && flat_oriented && (lds_f4 + 8 * ostride_f4) * sizeof(float4) <= small_image_bytes) {
        info.flat_ostride = (uint32_t)ostride_f4;
        lds_f4 += 8 * ostride_f4;
    }
    info.flat_rank = lds_f4;
    info.pnodes = info.flat_rank + (flat_ok ? 32 : 0);
    info.prim_rank = info.pnodes + 2ull * n_pnodes;
    info.wnodes = info.prim_rank + (8ull * n_prims + 3) / 4;
    info.n_float4 = info.wnodes + 8ull * wide.size();
    info.n_nodes = n_nodes; info.n_prims = n_prims; info.n_tris = in.n_triangles; info.n_materials = in.n_materials;
    info.n_spheres = in.n_spheres; info.n_planes = in.n_planes;
    info.n_leaves = (uint32_t)leaf_nodes.size(); info.n_pnodes = n_pnodes; info.n_wnodes = (uint32_t)wide.size();
    info.tri_mask_lo = (uint32_t)tri_mask; info.tri_mask_hi = (uint32_t)(tri_mask >> 32);
    info.plane_mask_lo = (uint32_t)plane_mask; info.plane_mask_hi = (uint32_t)(plane_mask >> 32);
    info.flat_ok = flat_ok ? 1u : 0u;
    info.typed_leaves = typed_leaves ? 1u : 0u;
    info.wide_ok = wide_ok ? 1u : 0u;
    info.wide_deep = (wide_ok && wide_depth > RT_WSTACK + 1u) ? 1u : 0u;
    info.coop_ok = (wide_ok && n_prims < RT_COOP_MAX_RECORDS && wide.size() < RT_COOP_MAX_NODES) ? 1u : 0u; // (build_wide_tree already bounds the depth at 25 wide levels)
    info.stack_entries = depth + 1;
    info.lds_float4s = (lds_f4 * sizeof(float4) <= small_image_bytes) ? (uint32_t)lds_f4 : 0u; // whole image in LDS only while it leaves room for the path pools
    info.cull_always = 0xffffffffu;
    if (flat_ok) fill_cull_groups(nodes, leaf_index, info);
    info.top_elems = pl.top_elems;
    info.wimg_nodes = wide_ok ? (uint32_t)wide.size() : 0u; // the wide walks' LDS image is the head of the wide-node array (hottest first), as far as the launch's room goes (hybrid_stage)
    info.small_image_bytes = (uint32_t)small_image_bytes;
    info.hybrid_room_f4 = hybrid_room_f4;
    // ---- the sections
    std::vector<float4> &img = out.image;
    img.resize(info.n_float4);
    float4 *p_nodes = img.data() + info.nodes;
    for (uint32_t i = 0; i < n_nodes; i++) {
        const rsrt_bvh_node &nd = nodes[i];
        uint32_t hi = nd.split_axis; // interior: split axis; leaf (when every leaf has <= 8 primitives): triangle mask | plane mask << 8
        if (nd.primitives_len != 0) {
            hi = 0;
            if (typed_leaves)
                for (uint32_t k = 0; k < nd.primitives_len; k++) {
                    const uint32_t ty = prims[first_record(nd) + k].primitive_type;
                    if (ty >= 2) hi |= 1u << k;
                    else if (ty == 1) hi |= 1u << (8 + k);
                }
        }
        p_nodes[2 * i] = f4(nd.bounds_min[0], nd.bounds_min[1], nd.bounds_min[2], u2f(nd.primitives_or_second_child_index));
        p_nodes[2 * i + 1] = f4(nd.bounds_max[0], nd.bounds_max[1], nd.bounds_max[2], u2f(nd.primitives_len | (hi << 16)));
    }
    memcpy(img.data() + info.escape, escape.data(), escape.size() * sizeof(uint32_t));
    float4 *p_prims = img.data() + info.prims;
    for (uint32_t i = 0; i < n_prims; i++) {
        const rsrt_primitive_info &pi = prims[i];
        if (pi.primitive_type == 0) make_sphere_record(in.spheres[pi.index], p_prims + 4 * i);
        else if (pi.primitive_type == 1) make_plane_record(in.planes[pi.index], p_prims + 4 * i);
        else make_triangle_record(in.triangles[pi.index], pi.index, in.vertices, p_prims + 4 * i);
    }
    for (uint32_t i = 0; i < in.n_triangles; i++) {
        const rsrt_triangle &t = in.triangles[i];
        const float *a = in.normals[t.normal_0].v, *b = in.normals[t.normal_1].v, *c = in.normals[t.normal_2].v;
        float4 *p = img.data() + info.tri_normals + 3 * i;
        p[0] = f4(a[0], a[1], a[2], b[0]);
        p[1] = f4(b[1], b[2], c[0], c[1]);
        p[2] = f4(c[2], 0, 0, 0);
    }
    for (uint32_t i = 0; i < in.n_materials; i++) make_material_record(in.materials[i], img.data() + info.materials + 4 * i);
    for (uint32_t i = 0; i < in.n_spheres; i++) make_sphere_record(in.spheres[i], img.data() + info.fb_spheres + 4 * i);
    for (uint32_t i = 0; i < in.n_planes; i++) make_plane_record(in.planes[i], img.data() + info.fb_planes + 4 * i);
    // A record whose geometry is bit for bit that of an EARLIER record of the same leaf can never win: it gives the very same t to
    // every ray, and the reference keeps the first of equals (strict <, a leaf's records in index order whatever the octant) —
    // house.toml lists its ground plane twice.  The flat loop leaves such a record out of its leaf's mask.  The cooperative walk
    // (rt_coop.h), which folds an extension ray's hits with an atomic minimum and sends a ray that sees two records at the same
    // closest t through the exact walk once more, finds it marked in a word no test reads (r2.w) and counts it as a miss, so that
    // doubled geometry does not make every hit a tie.
    std::vector<uint32_t> twins;
    for (uint32_t i : leaf_nodes)
        for (uint32_t b = 1; b < nodes[i].primitives_len; b++)
            for (uint32_t a = 0; a < b; a++)
                if (same_test(p_prims + 4 * (first_record(nodes[i]) + a), p_prims + 4 * (first_record(nodes[i]) + b))) {
                    twins.push_back(first_record(nodes[i]) + b);
                    break;
                }
    if (flat_ok) {
        uint64_t twin_mask = 0;
        for (uint32_t r : twins) twin_mask |= 1ull << r;
        float4 *p_flat = img.data() + info.flat_leaves;
        for (size_t k = 0; k < leaf_nodes.size(); k++) {
            const rsrt_bvh_node &nd = nodes[leaf_nodes[k]];
            const uint64_t lm = ((nd.primitives_len >= 64 ? ~0ull : ((1ull << nd.primitives_len) - 1ull)) << first_record(nd)) & ~twin_mask;
            p_flat[2 * k] = f4(nd.bounds_min[0], nd.bounds_min[1], nd.bounds_min[2], u2f((uint32_t)lm));
            p_flat[2 * k + 1] = f4(nd.bounds_max[0], nd.bounds_max[1], nd.bounds_max[2], u2f((uint32_t)(lm >> 32)));
        }
        if (info.flat_ostride)
            for (uint32_t q = 0; q < 8; q++)
                for (size_t k = 0; k < leaf_nodes.size(); k++) {
                    const float4 lo = p_flat[2 * k], hi = p_flat[2 * k + 1];
                    float4 *c = p_flat + 2 * leaf_nodes.size() + q * ostride_f4 + 2 * k;
                    c[0] = f4(q & 1u ? hi.x : lo.x, q & 2u ? hi.y : lo.y, q & 4u ? hi.z : lo.z, lo.w);
                    c[1] = f4(q & 1u ? lo.x : hi.x, q & 2u ? lo.y : hi.y, q & 4u ? lo.z : hi.z, hi.w);
                }
        memcpy(img.data() + info.flat_rank, flat_rank, sizeof flat_rank);
    }
    for (uint32_t r : twins) p_prims[4 * r + 2].w = u2f(1u); // (after the masks: same_test compares these words too)
    std::vector<uint32_t> new_id(n_nodes + 1, n_pnodes); // old node -> element; [n_nodes] = end
    for (uint32_t e = 0; e < n_pnodes; e++)
        if (pl.elems[e].old != 0xffffffffu) new_id[pl.elems[e].old] = e;
    float4 *p_pnodes = img.data() + info.pnodes;
    for (uint32_t e = 0; e < n_pnodes; e++) {
        if (pl.elems[e].old == 0xffffffffu) { // jump element: both links equal, box never looked at
            const uint32_t to = new_id[pl.elems[e].jump_to];
            p_pnodes[2 * e] = p_pnodes[2 * e + 1] = f4(0, 0, 0, u2f(to));
            continue;
        }
        const uint32_t i = pl.elems[e].old;
        p_pnodes[2 * e] = p_nodes[2 * i];
        p_pnodes[2 * e + 1] = p_nodes[2 * i + 1];
        if (nodes[i].primitives_len == 0) { // interior: {min, link when hit}{max, link when missed}
            p_pnodes[2 * e].w = u2f(new_id[i + 1]);
            p_pnodes[2 * e + 1].w = u2f(new_id[pl.succ[i]]);
        } else { // leaf: first record | leaf flag; length | triangle mask << 16 | plane mask << 24 (as in `nodes`)
            p_pnodes[2 * e].w = u2f(first_record(nodes[i]) | 0x80000000u);
        }
    }
    if (n_prims) memcpy(img.data() + info.prim_rank, prim_rank.data(), prim_rank.size() * sizeof(uint32_t));
    fill_wide_nodes(wide, nodes, prims, img.data() + info.wnodes);
    return out;
}

} // namespace
