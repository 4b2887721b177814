// rt_video.h — the video pass's kernel and its C-ABI (include/rsrt.h "video output").  Included at the end of
// rsrt_api.hip.  All arithmetic is include/rsrt_video.h's.
//
//  rt_display_video_kernel<STD, DEPTH, SITING, LEVELS>
//      rt_display_colour_kernel's geometry: a 256-thread workgroup owns a tile of RT_LC_TW x RT_LC_TH = 32 x 8 pixels, its inputs
//      gathered by rt_display_gather from the same DisplayChain (rt_local.h).  The tile is even both ways and begins at even
//      coordinates, so a chroma quad never straddles workgroups: a tile holds 16 x 4 chroma samples.  Every lane runs the chain at its
//      pixel — clamped to the picture, so a lane past the edge holds the edge pixel's values, which is what the header's clamped taps
//      read there, and no lane leaves before the exchanges — forms Y', Cb', Cr' and stores its luma code.
//      SITING = CENTRE: a wave64 is two picture rows of 32, so a quad is lanes l, l ^ 1, l ^ 32, l ^ 33: the row's pair by
//      __shfl_xor 1, the two rows by __shfl_xor 32, and the quad's even-even lane quantises and stores.  No LDS, no barrier.
//      SITING = LEFT, TOPLEFT: every lane stages Cb', Cr' in LDS, two planes of 9 x 33 floats with a one-pixel apron on the left and (of
//      which only TOPLEFT fills and reads it) on the top; the apron is 8 (LEFT) or 8 + 33 (TOPLEFT) further chain evaluations by the
//      first lanes, at clamped coordinates as the finished display's ring makes them.  One __syncthreads, then the 64 lanes of wave 0
//      filter [1 2 1] / 4 along x, average or filter along y, quantise and store one chroma sample each.  Their LDS reads are 4-byte
//      reads at a stride of two floats, two lanes a bank: 2 cycles more a read, eighteen reads a workgroup.
//      Stores: one luma sample a lane, a byte or a uint16 (a row of the tile is 32 or 64 contiguous bytes); a semi-planar chroma pair as
//      one 2- or 4-byte word where the plane's start is aligned for it (W x H even), else as two samples.  Packing four luma samples
//      into one word across lanes (three __shfl_down, every fourth lane stores) was built and measured too: not faster.
//      LEVELS (STD = HDR10): rt_display_hdr_kernel's reduction of q = rsrt_hdr_level_q of the same nits into the workgroup's pair
//      {sum q, max q}, summed by rt_hdr_levels_kernel (rt_hdr.h).
//      STD and DEPTH fix the tables, the matrix and the sample's width at compile time; range, layout and dither are read at run time.
//      No scratch memory in any variant.
//  The entry point's checks are display_chain's (rt_local.h); its own are levels_out's and the choice of the variant.

#define RT_VD_SW (RT_LC_TW + 1) // staged values a row: the apron's column, then the tile's
#define RT_VD_SH (RT_LC_TH + 1) // rows: the apron's, then the tile's
#define RT_VD_CW (RT_LC_TW / 2) // chroma samples of a tile
#define RT_VD_CH (RT_LC_TH / 2)

static_assert(RT_LC_TW % 2 == 0 && RT_LC_TH % 2 == 0 && RT_LC_TW * 2 == RT_WAVE, "a quad lies in one workgroup, and a wave is two rows of the tile");
static_assert(RT_VD_CW * RT_VD_CH == RT_WAVE && RT_LC_TH + RT_VD_SW <= RT_LC_BLOCK, "one wave filters the tile's chroma; the apron is one round of the workgroup");

template <uint32_t DEPTH>
__device__ __forceinline__ void rt_video_store(unsigned char *plane, size_t i, uint32_t word)
{
    if constexpr (DEPTH == 10u) reinterpret_cast<uint16_t *>(plane)[i] = (uint16_t)word; else plane[i] = (unsigned char)word;
}

// hp: passed rsrt_hdr_params_ok with RSRT_HDR_PQ10 (STD = RSRT_VIDEO_HDR10; not looked at otherwise); vp: passed rsrt_video_params_ok,
// standard STD, depth DEPTH, siting SITING; out: a frame of rsrt_video_planes(c.w, c.h, vp); pairs: as rt_display_hdr_kernel's
template <uint32_t STD, uint32_t DEPTH, uint32_t SITING, bool LEVELS>
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_display_video_kernel(DisplayChain c, rsrt_hdr_params hp, rsrt_video_params vp, unsigned char *out, uint2 *pairs)
{
    vp.standard = STD; vp.depth = DEPTH; vp.siting = SITING; // (what the variant was chosen by: known to the compiler)
    const int w = c.w, h = c.h;
    const auto ycc_at = [&c, &hp](int px, int py, float ycc[3], uint32_t *q) { // steps 1 to 3 at a pixel of the picture
        float sum[3], gain, v[3], e[3];
        rsrt_bloom_rgb up_b;
        rt_display_gather(c, c.graded, px, py, sum, &gain, &up_b);
        if constexpr (STD == RSRT_VIDEO_HDR10) {
            rsrt_hdr_pixel_nits(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, &hp, v);
            if (LEVELS && q) *q = rsrt_hdr_level_q(v);
        } else {
            rsrt_finish_sdr(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, reinterpret_cast<const float *>(c.lut), c.n, v);
        }
        rsrt_video_signal(STD, v, e);
        rsrt_video_ycc(STD, e, ycc);
    };
    const int tid = (int)threadIdx.x, lx = tid % RT_LC_TW, ly = tid / RT_LC_TW;
    const int bx = (int)blockIdx.x * RT_LC_TW, by = (int)blockIdx.y * RT_LC_TH, x = bx + lx, y = by + ly;
    const bool in = x < w && y < h;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const size_t luma_bytes = (size_t)w * (size_t)h * (DEPTH == 10u ? 2u : 1u), chroma_bytes = (size_t)cw * (size_t)ch * (DEPTH == 10u ? 2u : 1u);
    const bool pair_ok = (((size_t)w * (size_t)h) & 1u) == 0u; // a pair's word is aligned in the interleaved plane
    const auto store_chroma = [&](int gx, int gy, float cb, float cr) { // step 5 and 6 of chroma sample (gx, gy) < (cw, ch)
        uint32_t codes[2];
        rsrt_video_chroma_codes(cb, cr, (uint32_t)gx, (uint32_t)gy, &vp, codes);
        const uint32_t b = rsrt_video_word(codes[0], &vp), r = rsrt_video_word(codes[1], &vp);
        const size_t i = (size_t)gy * (size_t)cw + (size_t)gx;
        unsigned char *const plane = out + luma_bytes;
        if (vp.layout == RSRT_VIDEO_PLANAR) {
            rt_video_store<DEPTH>(plane, i, b);
            rt_video_store<DEPTH>(plane + chroma_bytes, i, r);
        } else if (pair_ok) {
            if constexpr (DEPTH == 10u) reinterpret_cast<uint32_t *>(plane)[i] = b | r << 16; else reinterpret_cast<uint16_t *>(plane)[i] = (uint16_t)(b | r << 8);
        } else {
            rt_video_store<DEPTH>(plane, 2u * i, b);
            rt_video_store<DEPTH>(plane, 2u * i + 1u, r);
        }
    };
    float ycc[3];
    uint32_t q = 0u;
    ycc_at(x < w ? x : w - 1, y < h ? y : h - 1, ycc, &q);
    if (!in) q = 0u;
    if (in) rt_video_store<DEPTH>(out, (size_t)y * (size_t)w + (size_t)x, rsrt_video_word(rsrt_video_luma_code(ycc[0], (uint32_t)x, (uint32_t)y, &vp), &vp));
    if constexpr (SITING == RSRT_VIDEO_SITING_CENTRE) {
        // (every lane of the wave is here: lanes past the picture hold the clamped pixel's values)
        const float rb = ycc[1] + __shfl_xor(ycc[1], 1, RT_WAVE), rr = ycc[2] + __shfl_xor(ycc[2], 1, RT_WAVE); // p00 + p01, and p10 + p11 a row below
        const float cb = (rb + __shfl_xor(rb, RT_LC_TW, RT_WAVE)) * 0.25f, cr = (rr + __shfl_xor(rr, RT_LC_TW, RT_WAVE)) * 0.25f;
        if (in && lx % 2 == 0 && ly % 2 == 0) store_chroma(x / 2, y / 2, cb, cr);
    } else {
        __shared__ float s_cb[RT_VD_SH * RT_VD_SW], s_cr[RT_VD_SH * RT_VD_SW]; // [(sy + 1) * RT_VD_SW + sx + 1]: pixel (bx + sx, by + sy), clamped to the picture
        s_cb[(ly + 1) * RT_VD_SW + lx + 1] = ycc[1];
        s_cr[(ly + 1) * RT_VD_SW + lx + 1] = ycc[2];
        if (tid < (SITING == RSRT_VIDEO_SITING_TOPLEFT ? RT_LC_TH + RT_VD_SW : RT_LC_TH)) { // the column to the left, then the row above with its corner
            const int sx = tid < RT_LC_TH ? -1 : tid - RT_LC_TH - 1, sy = tid < RT_LC_TH ? tid : -1;
            int px = bx + sx, py = by + sy;
            px = px < 0 ? 0 : (px < w ? px : w - 1);
            py = py < 0 ? 0 : (py < h ? py : h - 1);
            float a[3];
            ycc_at(px, py, a, nullptr);
            s_cb[(sy + 1) * RT_VD_SW + sx + 1] = a[1];
            s_cr[(sy + 1) * RT_VD_SW + sx + 1] = a[2];
        }
        __syncthreads();
        const int ccx = tid % RT_VD_CW, ccy = tid / RT_VD_CW, gx = bx / 2 + ccx, gy = by / 2 + ccy;
        if (tid < RT_VD_CW * RT_VD_CH && gx < cw && gy < ch) {
            const int col = 2 * ccx + 1; // of pixel 2 gx; its neighbours col - 1 and col + 1 <= RT_LC_TW
            const auto h121 = [col](const float *s, int sy) { return rsrt_video_h121(s[(sy + 1) * RT_VD_SW + col - 1], s[(sy + 1) * RT_VD_SW + col], s[(sy + 1) * RT_VD_SW + col + 1]); };
            float cb, cr;
            if constexpr (SITING == RSRT_VIDEO_SITING_LEFT) {
                cb = rsrt_video_left(h121(s_cb, 2 * ccy), h121(s_cb, 2 * ccy + 1));
                cr = rsrt_video_left(h121(s_cr, 2 * ccy), h121(s_cr, 2 * ccy + 1));
            } else {
                cb = rsrt_video_h121(h121(s_cb, 2 * ccy - 1), h121(s_cb, 2 * ccy), h121(s_cb, 2 * ccy + 1));
                cr = rsrt_video_h121(h121(s_cr, 2 * ccy - 1), h121(s_cr, 2 * ccy), h121(s_cr, 2 * ccy + 1));
            }
            store_chroma(gx, gy, cb, cr);
        }
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

namespace {

using VideoKernel = void (*)(DisplayChain, rsrt_hdr_params, rsrt_video_params, unsigned char *, uint2 *);

template <uint32_t STD, uint32_t DEPTH, bool LEVELS>
VideoKernel video_kernel_at(uint32_t siting)
{
    return siting == RSRT_VIDEO_SITING_CENTRE    ? rt_display_video_kernel<STD, DEPTH, RSRT_VIDEO_SITING_CENTRE, LEVELS>
           : siting == RSRT_VIDEO_SITING_TOPLEFT ? rt_display_video_kernel<STD, DEPTH, RSRT_VIDEO_SITING_TOPLEFT, LEVELS>
                                                 : rt_display_video_kernel<STD, DEPTH, RSRT_VIDEO_SITING_LEFT, LEVELS>;
}

} // namespace

extern "C" {

rsrt_status rsrt_display_video(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local, float bloom_intensity,
                               const rsrt_colour_params *colour, const rsrt_hdr_params *hdr, const rsrt_video_params *video, void *host_out, size_t n_bytes,
                               rsrt_hdr_levels *levels_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    DisplayChain c;
    rsrt_status st = display_chain(ctx, "display_video", CHAIN_COLOUR | CHAIN_VIDEO, source, sample_total, exposure, local, colour, nullptr, hdr, bloom_intensity, host_out,
                                   n_bytes, &c, video);
    if (st) return st;
    const bool hdr10 = video->standard == RSRT_VIDEO_HDR10, lv = levels_out != nullptr;
    if (lv && !hdr10) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_video: levels_out must be NULL for RSRT_VIDEO_BT709 (content light levels are HDR10's)");
    const VideoKernel kernel = hdr10 ? (lv ? video_kernel_at<RSRT_VIDEO_HDR10, 10u, true>(video->siting) : video_kernel_at<RSRT_VIDEO_HDR10, 10u, false>(video->siting))
                               : video->depth == 10u ? video_kernel_at<RSRT_VIDEO_BT709, 10u, false>(video->siting)
                                                     : video_kernel_at<RSRT_VIDEO_BT709, 8u, false>(video->siting);
    const dim3 tiles = display_tiles(c);
    const size_t n_pairs = (size_t)tiles.x * tiles.y;
    const size_t at = (n_bytes + 15u) & ~(size_t)15u; // where the levels' 16 bytes lie in the scratch buffer; the pairs follow them
    unsigned long long words[2] = {0ull, 0ull};
    st = read_back(ctx, host_out, n_bytes, lv ? at - n_bytes + RT_HDR_LEVEL_BYTES + n_pairs * sizeof(uint2) : 0, [&](void *tmp) {
        unsigned long long *const dev = lv ? reinterpret_cast<unsigned long long *>(static_cast<char *>(tmp) + at) : nullptr;
        uint2 *const pairs = lv ? reinterpret_cast<uint2 *>(dev + 2) : nullptr;
        kernel<<<tiles, dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, hdr10 ? *hdr : rsrt_hdr_params{}, *video, static_cast<unsigned char *>(tmp), pairs);
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
