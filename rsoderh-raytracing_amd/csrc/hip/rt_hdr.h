// rt_hdr.h — the HDR display's kernels and its C-ABI (include/rsrt.h "HDR display").  Included at the end of
// rsrt_api.hip.  All arithmetic is include/rsrt_hdr.h's.
//
//  rt_display_hdr_kernel<ENC, LEVELS>  rt_display_colour_kernel's geometry — a 256-thread workgroup owns a tile of RT_LC_TW x RT_LC_TH
//                                      pixels, one thread a pixel, its inputs gathered by rt_display_gather from the same DisplayChain
//                                      (rt_local.h) — with rsrt_hdr_pixel_nits in the place of the tone map and one of two tails:
//                                      ENC = RSRT_HDR_PQ10 packs three 10-bit codes (three 10-step searches of the 4 KB threshold table,
//                                      which the caches serve) and stores 4 bytes a lane, a wave's row of 32 lanes 128 contiguous bytes;
//                                      ENC = RSRT_HDR_SCRGB16F stores four halfs as one 8-byte word a lane, 256 contiguous bytes a row.
//                                      No LDS and no barrier without LEVELS; no scratch memory in any variant.
//                                      LEVELS: every lane holds q = rsrt_hdr_level_q of its pixel (0 outside the picture: such lanes
//                                      stay until the barrier).  max q and sum q go down the wave64 with __shfl_xor in 32 bits — a
//                                      workgroup's sum is at most 256 * 640000 < 2^32 — then lane 0 of each of the four waves stores
//                                      its pair in LDS (two 4-byte stores: nothing wide to serialise), one __syncthreads, and thread 0
//                                      writes the workgroup's pair {sum q, max q} to its own 8 bytes of device scratch with a plain
//                                      store, zeros included: nothing to clear in front of a call.
//  rt_hdr_levels_kernel                one workgroup: the pairs' sum (64 bits) and maximum, down the waves and through LDS the same way,
//                                      into the call's 16 bytes.  Integers only: no order of anything changes the result.
//                                      (One atomicAdd and one atomicMax a workgroup into those 16 bytes instead of the pairs was built
//                                      first and measured: the 8100 workgroups of a 1920 x 1080 frame meet in two words, device-wide
//                                      atomics on one address are served one after the other, and the kernel took four times as long:
//                                      DESIGN.md §25.)
//  The entry point's checks are display_chain's (rt_local.h); its own are the choice of the variant and the levels' copy.

#define RT_HDR_LEVEL_BYTES 16u // {uint64 sum q, uint32 max q, uint32 zero} behind the picture in the scratch buffer, 16-byte aligned; the pairs follow

static_assert((unsigned long long)RT_LC_BLOCK * (unsigned long long)(RSRT_HDR_MAX_NITS * RSRT_HDR_LEVEL_SCALE) < 0xffffffffull, "a workgroup's sum of q fits 32 bits");

// max and sum of a wave's 64 values, in every lane
__device__ __forceinline__ void rt_hdr_wave_reduce(uint32_t &mx, uint32_t &sm)
{
#pragma unroll
    for (int off = RT_WAVE / 2; off > 0; off >>= 1) {
        const uint32_t omx = (uint32_t)__shfl_xor((int)mx, off, RT_WAVE), osm = (uint32_t)__shfl_xor((int)sm, off, RT_WAVE);
        mx = mx > omx ? mx : omx;
        sm += osm;
    }
}

// hp: passed rsrt_hdr_params_ok, hp.encoding == ENC; pairs: written only with LEVELS, one {sum q, max q} a workgroup, row-major over the grid
template <uint32_t ENC, bool LEVELS>
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_hdr_kernel(DisplayChain c, rsrt_hdr_params hp, void *out, uint2 *pairs)
{
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * RT_LC_TW + tid % RT_LC_TW, y = (int)blockIdx.y * RT_LC_TH + tid / RT_LC_TW;
    const bool in = x < c.w && y < c.h;
    if (!LEVELS && !in) return;
    uint32_t q = 0u;
    if (in) {
        float sum[3], gain, nits[3];
        rsrt_bloom_rgb up_b;
        rt_display_gather(c, c.graded, x, y, sum, &gain, &up_b);
        rsrt_hdr_pixel_nits(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, &hp, nits);
        const size_t i = (size_t)y * (size_t)c.w + (size_t)x;
        if constexpr (ENC == RSRT_HDR_PQ10) {
            static_cast<uint32_t *>(out)[i] = rsrt_hdr_pack_pq10(nits, (uint32_t)x, (uint32_t)y, &hp);
        } else {
            uint16_t half[4];
            rsrt_hdr_pack_scrgb(nits, half);
            static_cast<uint2 *>(out)[i] = make_uint2((uint32_t)half[0] | (uint32_t)half[1] << 16, (uint32_t)half[2] | (uint32_t)half[3] << 16);
        }
        if constexpr (LEVELS) q = rsrt_hdr_level_q(nits);
    }
    if constexpr (LEVELS) {
        __shared__ uint32_t wave_max[RT_LC_BLOCK / RT_WAVE], wave_sum[RT_LC_BLOCK / RT_WAVE];
        uint32_t mx = q, sm = q;
        rt_hdr_wave_reduce(mx, sm);
        if (tid % RT_WAVE == 0) {
            wave_max[tid / RT_WAVE] = mx;
            wave_sum[tid / RT_WAVE] = sm;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t bmx = 0u, bsm = 0u;
#pragma unroll
            for (int k = 0; k < RT_LC_BLOCK / RT_WAVE; k++) {
                bmx = bmx > wave_max[k] ? bmx : wave_max[k];
                bsm += wave_sum[k];
            }
            pairs[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = make_uint2(bsm, bmx);
        }
    }
}

// n pairs {sum q, max q} -> levels[0] = the sum of the sums, levels[1] = the largest maximum (its high word 0); one workgroup
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_hdr_levels_kernel(const uint2 *pairs, uint32_t n, unsigned long long *levels)
{
    __shared__ unsigned long long wave_sum[RT_LC_BLOCK / RT_WAVE];
    __shared__ uint32_t wave_max[RT_LC_BLOCK / RT_WAVE];
    const uint32_t tid = threadIdx.x;
    unsigned long long sm = 0ull;
    uint32_t mx = 0u;
    for (uint32_t i = tid; i < n; i += RT_LC_BLOCK) { // (n is the workgroup's: every lane reaches the shuffles)
        const uint2 p = pairs[i];
        sm += p.x;
        mx = mx > p.y ? mx : p.y;
    }
#pragma unroll
    for (int off = RT_WAVE / 2; off > 0; off >>= 1) { // the 64-bit sum as its two halves
        const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)sm, off, RT_WAVE), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(sm >> 32), off, RT_WAVE);
        const uint32_t omx = (uint32_t)__shfl_xor((int)mx, off, RT_WAVE);
        sm += (unsigned long long)ohi << 32 | olo;
        mx = mx > omx ? mx : omx;
    }
    if (tid % RT_WAVE == 0) {
        wave_sum[tid / RT_WAVE] = sm;
        wave_max[tid / RT_WAVE] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0ull;
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < RT_LC_BLOCK / RT_WAVE; k++) {
            s += wave_sum[k];
            m = m > wave_max[k] ? m : wave_max[k];
        }
        levels[0] = s;
        levels[1] = m;
    }
}

extern "C" {

rsrt_status rsrt_display_hdr(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local, float bloom_intensity,
                             const rsrt_colour_params *colour, const rsrt_hdr_params *hdr, void *host_out, size_t n_bytes, rsrt_hdr_levels *levels_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    DisplayChain c;
    rsrt_status st = display_chain(ctx, "display_hdr", CHAIN_COLOUR | CHAIN_HDR, source, sample_total, exposure, local, colour, nullptr, hdr, bloom_intensity, host_out,
                                   n_bytes, &c);
    if (st) return st;
    const bool pq = hdr->encoding == RSRT_HDR_PQ10, lv = levels_out != nullptr;
    const auto kernel = pq ? (lv ? rt_display_hdr_kernel<RSRT_HDR_PQ10, true> : rt_display_hdr_kernel<RSRT_HDR_PQ10, false>)
                           : (lv ? rt_display_hdr_kernel<RSRT_HDR_SCRGB16F, true> : rt_display_hdr_kernel<RSRT_HDR_SCRGB16F, false>);
    const dim3 tiles = display_tiles(c);
    const size_t n_pairs = (size_t)tiles.x * tiles.y;
    const size_t at = (n_bytes + 15u) & ~(size_t)15u; // where the levels' 16 bytes lie in the scratch buffer; the pairs follow them
    unsigned long long words[2] = {0ull, 0ull};
    st = read_back(ctx, host_out, n_bytes, lv ? at - n_bytes + RT_HDR_LEVEL_BYTES + n_pairs * sizeof(uint2) : 0, [&](void *tmp) {
        unsigned long long *const dev = lv ? reinterpret_cast<unsigned long long *>(static_cast<char *>(tmp) + at) : nullptr;
        uint2 *const pairs = lv ? reinterpret_cast<uint2 *>(dev + 2) : nullptr;
        kernel<<<tiles, dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, *hdr, tmp, pairs);
        if (lv) {
            rt_hdr_levels_kernel<<<dim3(1), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(pairs, (uint32_t)n_pairs, dev);
            HIP_TRY(ctx, hipMemcpyAsync(words, dev, RT_HDR_LEVEL_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        }
        return RSRT_OK;
    });
    if (st) return st;
    if (lv) rsrt_hdr_levels_from((uint32_t)words[1], (uint64_t)words[0], (uint64_t)c.w * (uint64_t)c.h, levels_out);
    return RSRT_OK;
}

} // extern "C"
