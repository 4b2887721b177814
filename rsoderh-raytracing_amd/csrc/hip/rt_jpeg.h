// rt_jpeg.h — the JPEG pass's kernels and its C-ABI (include/rsrt.h "JPEG output").  Included at the end of
// rsrt_api.hip.  All arithmetic is include/rsrt_jpeg.h's.  Everywhere a wave64 is one 8 x 8 block and a lane one of its 64 values.
//
//  rt_jpeg_blocks_kernel<SUBSAMPLING>
//      256 threads, four waves.  RSRT_JPEG_420: a workgroup is one MCU of 16 x 16 pixels, wave k its luma block Yk, lane (ly, lx) the
//      block's pixel; RSRT_JPEG_444: a workgroup is four MCUs of one MCU row, wave k the k-th.  Every lane runs the chain at its pixel —
//      clamped to the picture, so a lane past the edge holds the edge pixel's samples, which is what the header's clamped taps read
//      there — through rt_display_gather, as the colour and video kernels do, and forms sY, sCb, sCr.
//      The DCT needs no LDS: a lane's eight taps of the first pass are its row's lanes and of the second its column's, sixteen
//      ds_bpermute a block (__shfl), each a broadcast inside eight lanes; lane (y, u) holds t[y][u] after the first pass and c[v = y][u]
//      after the second.  The quantiser's divisor is computed in the lane (integers, a division by a constant); the zigzag is one more
//      __shfl by the table of lane indices, after which lane k holds coefficient k.
//      4:2:0 chroma: a 2 x 2 quad lies in one wave's block (lanes l, l ^ 1, l ^ 8), reduced by two __shfl_xor as the video pass's centre
//      siting does; the even-even lanes store the wave's 4 x 4 quarter of the MCU's Cb and Cr blocks into 2 x 64 floats of LDS, one
//      __syncthreads, and waves 0 and 1 transform them.  4:4:4 uses no LDS and no barrier.
//      It writes the block's 64 int16 (128 contiguous bytes a wave) and one word a block: the bits of its AC code and EOB in the low
//      half, its DC in the high half.
//  DC prediction: a block's predecessor belongs to another workgroup, so the DCs are written first and the differences are taken
//      afterwards — by the scan for the bit count, by the packer for the code — from that word and rsrt_jpeg_block_pred's index
//      arithmetic.  The other way, a workgroup owning a run of MCUs, would serialise the chain evaluations of a run inside one
//      workgroup for the sake of one subtraction a block; the word costs 4 bytes a block.
//  rt_jpeg_count_kernel   the same word from uploaded coefficients (rsrt_jpeg_encode_coefficients).
//  rt_jpeg_scan_kernel    one workgroup: the exclusive prefix sum of the blocks' bit counts (AC bits + the DC difference's code) into
//      uint32 bit offsets, 256 blocks a round (a wave scan by __shfl_up, the four waves' sums through LDS), and the total.
//  rt_jpeg_pack_kernel    a wave a block.  The non-zero ACs are one __ballot; a lane's run is the distance to the previous set bit; its
//      code (ZRLs, symbol, value: at most 59 bits) and length come from rsrt_jpeg_ac_code, the DC lane's from rsrt_jpeg_dc_code, and lane
//      63 carries the EOB when its coefficient is zero.  A wave prefix sum places every lane's code; the lanes OR them into the wave's
//      zeroed LDS words (ds_or_b32; a code touches up to three), and the words go to the scan at the block's bit offset in the file's
//      byte order: interior words by plain stores, the first and the last, which neighbours share, by atomicOr into the zeroed scan.
//      OR commutes: the bytes do not depend on any order.  Vector stores and vector atomics only.
//  No scratch memory in any kernel.
//  The host reads the total (8 bytes), copies ceil(bits / 8) bytes of scan (read_back_counted) and writes headers, stuffed scan, padding
//  and EOI with the header's inline functions.

#define RT_JP_WAVES (RT_LC_BLOCK / RT_WAVE)
#define RT_JP_WORDS 56 // a block's words in LDS: 31 bits of the first word's other owner + 1658 are 53 words; a lane's third word may be two further

static_assert(RT_WAVE == 64 && RT_JP_WAVES == 4 && RT_JP_WORDS <= RT_WAVE && (31u + 1658u + 31u) / 32u + 2u <= RT_JP_WORDS, "a wave is a block; its lanes zero and store its words");
static_assert(RSRT_JPEG_BLOCK_BITS % 32u == 0u, "a block's slot is whole words");

// lane k's part of a block's code, k's coefficient v in every lane of the wave (all 64 call this): its bit count, the bits in *bits.
// Lane 0 codes dc_diff when with_dc, else nothing.
__device__ __forceinline__ uint32_t rt_jpeg_lane_code(int lane, int v, bool with_dc, int dc_diff, uint32_t chroma, uint64_t *bits)
{
    const unsigned long long mask = __ballot(v != 0 && lane > 0);
    *bits = 0u;
    if (lane == 0) return with_dc ? rsrt_jpeg_dc_code(dc_diff, chroma, bits) : 0u;
    if (v != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const int prev = below ? 63 - __clzll((long long)below) : 0; // (the DC's place when there is none)
        return rsrt_jpeg_ac_code((uint32_t)(lane - prev - 1), v, chroma, bits);
    }
    return lane == 63 ? rsrt_jpeg_eob_code(chroma, bits) : 0u;
}

// the inclusive prefix sum of v over the wave's lanes
__device__ __forceinline__ uint32_t rt_jpeg_wave_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int off = 1; off < RT_WAVE; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, off, RT_WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// a block's word from its coefficients, zz of lane k being coefficient k: AC bits (EOB with them) | DC << 16
__device__ __forceinline__ void rt_jpeg_store_word(int lane, int zz, uint32_t chroma, uint32_t *words, size_t block)
{
    uint64_t bits;
    const uint32_t sum = rt_jpeg_wave_scan(rt_jpeg_lane_code(lane, zz, false, 0, chroma, &bits), lane);
    const uint32_t dc = (uint32_t)__shfl(zz, 0, RT_WAVE); // (by every lane: an exchange reads no lane that is switched off)
    if (lane == RT_WAVE - 1) words[block] = sum | dc << 16;
}

// steps 4 and 5 of a block whose sample (y, x) lane y * 8 + x holds, and its outputs
__device__ __forceinline__ void rt_jpeg_emit(float s, int lane, uint32_t chroma, uint32_t quality, int16_t *coefs, uint32_t *words, size_t block)
{
    const int u = lane & 7, y = lane >> 3;
    float t = RSRT_JPEG_DCT[8 * u] * __shfl(s, y * 8, RT_WAVE);
#pragma unroll
    for (int k = 1; k < 8; k++) t = t + RSRT_JPEG_DCT[8 * u + k] * __shfl(s, y * 8 + k, RT_WAVE);
    float c = RSRT_JPEG_DCT[8 * y] * __shfl(t, u, RT_WAVE); // (v = y)
#pragma unroll
    for (int k = 1; k < 8; k++) c = c + RSRT_JPEG_DCT[8 * y + k] * __shfl(t, k * 8 + u, RT_WAVE);
    const int q = rsrt_jpeg_quantise(c, rsrt_jpeg_q_at((uint32_t)lane, chroma, quality), lane == 0);
    const int zz = __shfl(q, (int)RSRT_JPEG_ZIGZAG[lane], RT_WAVE);
    coefs[block * 64u + (size_t)lane] = (int16_t)zz;
    rt_jpeg_store_word(lane, zz, chroma, words, block);
}

// jp: passed rsrt_jpeg_params_ok, subsampling SUB; mw: MCUs a row; coefs: 64 int16 a block, words: one a block, in scan order
template <uint32_t SUB>
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_jpeg_blocks_kernel(DisplayChain c, uint32_t quality, uint32_t mw, int16_t *coefs, uint32_t *words)
{
    const int tid = (int)threadIdx.x, wave = tid / RT_WAVE, lane = tid % RT_WAVE, lx = lane & 7, ly = lane >> 3;
    const uint32_t mcu_x = SUB == RSRT_JPEG_444 ? blockIdx.x * RT_JP_WAVES + (uint32_t)wave : blockIdx.x;
    const int x0 = SUB == RSRT_JPEG_444 ? (int)mcu_x * 8 : (int)mcu_x * 16 + (wave & 1) * 8, y0 = SUB == RSRT_JPEG_444 ? (int)blockIdx.y * 8 : (int)blockIdx.y * 16 + (wave >> 1) * 8;
    const int px = x0 + lx < c.w ? x0 + lx : c.w - 1, py = y0 + ly < c.h ? y0 + ly : c.h - 1;
    float sum[3], gain, v[3], s[3];
    rsrt_bloom_rgb up_b;
    rt_display_gather(c, c.graded, px, py, sum, &gain, &up_b);
    rsrt_finish_sdr(sum, c.total, c.exposure, c.intensity, up_b, gain, &c.colour, reinterpret_cast<const float *>(c.lut), c.n, v);
    rsrt_jpeg_samples(v, s);
    if constexpr (SUB == RSRT_JPEG_444) {
        if (mcu_x >= mw) return; // (the whole wave: no barrier follows)
        const size_t first = ((size_t)blockIdx.y * mw + mcu_x) * 3u;
        rt_jpeg_emit(s[0], lane, 0u, quality, coefs, words, first);
        rt_jpeg_emit(s[1], lane, 1u, quality, coefs, words, first + 1u);
        rt_jpeg_emit(s[2], lane, 1u, quality, coefs, words, first + 2u);
    } else {
        __shared__ float s_c[2][64]; // the MCU's Cb and Cr blocks, [cy * 8 + cx]
        const size_t first = ((size_t)blockIdx.y * mw + mcu_x) * 6u;
        // (every lane of the wave is here: p00 + p01, then + (p10 + p11) a row below, in the quad's even-even lane)
        const float rb = s[1] + __shfl_xor(s[1], 1, RT_WAVE), rr = s[2] + __shfl_xor(s[2], 1, RT_WAVE);
        const float cb = (rb + __shfl_xor(rb, 8, RT_WAVE)) * 0.25f, cr = (rr + __shfl_xor(rr, 8, RT_WAVE)) * 0.25f;
        if ((lx & 1) == 0 && (ly & 1) == 0) {
            const int ci = ((wave >> 1) * 4 + (ly >> 1)) * 8 + (wave & 1) * 4 + (lx >> 1);
            s_c[0][ci] = cb;
            s_c[1][ci] = cr;
        }
        rt_jpeg_emit(s[0], lane, 0u, quality, coefs, words, first + (size_t)wave);
        __syncthreads();
        if (wave < 2) rt_jpeg_emit(s_c[wave][lane], lane, 1u, quality, coefs, words, first + 4u + (size_t)wave);
    }
}

__global__ __launch_bounds__(RT_LC_BLOCK) void rt_jpeg_count_kernel(const int16_t *coefs, uint32_t n, uint32_t subsampling, uint32_t *words)
{
    const int lane = (int)threadIdx.x % RT_WAVE;
    const size_t block = (size_t)blockIdx.x * RT_JP_WAVES + threadIdx.x / RT_WAVE;
    if (block >= n) return; // (the whole wave)
    rt_jpeg_store_word(lane, coefs[block * 64u + (size_t)lane], rsrt_jpeg_block_component(block, subsampling) ? 1u : 0u, words, block);
}

// block i's DC difference from the words
__device__ __forceinline__ int rt_jpeg_dc_diff(const uint32_t *words, size_t i, uint32_t subsampling)
{
    const int64_t pi = rsrt_jpeg_block_pred(i, subsampling);
    return (int)(int16_t)(words[i] >> 16) - (pi < 0 ? 0 : (int)(int16_t)(words[pi] >> 16));
}

// one workgroup.  offsets[i]: the bits of blocks 0 .. i - 1; *total: of all n (n * RSRT_JPEG_BLOCK_BITS < 2^32, the entry points' check)
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_jpeg_scan_kernel(const uint32_t *words, uint32_t n, uint32_t subsampling, uint32_t *offsets, unsigned long long *total)
{
    __shared__ uint32_t wave_sum[RT_JP_WAVES];
    const int tid = (int)threadIdx.x, wave = tid / RT_WAVE, lane = tid % RT_WAVE;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < n; base += RT_LC_BLOCK) { // (n is the workgroup's: every lane reaches the shuffles and the barriers)
        const uint32_t i = base + (uint32_t)tid;
        uint32_t bits = 0u;
        if (i < n) {
            uint64_t code;
            bits = (words[i] & 0xffffu) + rsrt_jpeg_dc_code(rt_jpeg_dc_diff(words, i, subsampling), rsrt_jpeg_block_component(i, subsampling) ? 1u : 0u, &code);
        }
        const uint32_t incl = rt_jpeg_wave_scan(bits, lane);
        if (lane == RT_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int k = 0; k < RT_JP_WAVES; k++) {
            before += k < wave ? wave_sum[k] : 0u;
            all += wave_sum[k];
        }
        if (i < n) offsets[i] = carry + before + (incl - bits);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// scan: zeroed, words of 32 bits whose memory order is the file's; n blocks' codes at offsets[]
__global__ __launch_bounds__(RT_LC_BLOCK) void rt_jpeg_pack_kernel(const int16_t *coefs, const uint32_t *words, const uint32_t *offsets, uint32_t n, uint32_t subsampling, uint32_t *scan)
{
    __shared__ uint32_t s_w[RT_JP_WAVES][RT_JP_WORDS]; // a wave's block from the word its first bit lies in; bit 31 of a word is its first
    const int wave = (int)threadIdx.x / RT_WAVE, lane = (int)threadIdx.x % RT_WAVE;
    const size_t block = (size_t)blockIdx.x * RT_JP_WAVES + (size_t)wave;
    const bool have = block < n;
    if (lane < RT_JP_WORDS) s_w[wave][lane] = 0u;
    __syncthreads();
    uint32_t off = 0u, total = 0u;
    if (have) { // (the whole wave)
        const uint32_t chroma = rsrt_jpeg_block_component(block, subsampling) ? 1u : 0u;
        uint64_t bits;
        const uint32_t len = rt_jpeg_lane_code(lane, coefs[block * 64u + (size_t)lane], true, rt_jpeg_dc_diff(words, block, subsampling), chroma, &bits);
        const uint32_t incl = rt_jpeg_wave_scan(len, lane);
        total = (uint32_t)__shfl((int)incl, RT_WAVE - 1, RT_WAVE);
        off = offsets[block];
        if (len) {
            const uint32_t pos = (off & 31u) + (incl - len), w0 = pos >> 5, b = pos & 31u;
            const uint64_t left = bits << (64u - len), a = left >> b; // the code from bit 63 down, then b bits into the first word
            const uint32_t a0 = (uint32_t)(a >> 32), a1 = (uint32_t)a, a2 = b ? (uint32_t)left << (32u - b) : 0u;
            if (a0) atomicOr(&s_w[wave][w0], a0);
            if (a1) atomicOr(&s_w[wave][w0 + 1u], a1);
            if (a2) atomicOr(&s_w[wave][w0 + 2u], a2);
        }
    }
    __syncthreads();
    if (have) {
        const uint32_t nw = ((off & 31u) + total + 31u) >> 5;
        if ((uint32_t)lane < nw) {
            const uint32_t word = __builtin_bswap32(s_w[wave][lane]);
            uint32_t *const at = scan + (off >> 5) + (uint32_t)lane;
            if (lane == 0 || (uint32_t)lane == nw - 1u) atomicOr(at, word); else *at = word;
        }
    }
}

namespace {

// where a call's pieces lie in the scratch buffer
struct JpegPlan {
    uint32_t w, h, mw, mh, n; // the picture, in pixels, MCUs and blocks
    size_t words_at, offsets_at, total_at, scan_at, scan_bytes, bytes; // (the coefficients lie at 0)
};

JpegPlan jpeg_plan(uint32_t w, uint32_t h, uint32_t subsampling)
{
    JpegPlan p;
    p.w = w; p.h = h;
    p.mw = rsrt_jpeg_mcus(w, subsampling); p.mh = rsrt_jpeg_mcus(h, subsampling);
    p.n = (uint32_t)rsrt_jpeg_blocks(w, h, subsampling);
    p.words_at = (size_t)p.n * 64u * sizeof(int16_t);
    p.offsets_at = p.words_at + (size_t)p.n * sizeof(uint32_t);
    p.total_at = (p.offsets_at + (size_t)p.n * sizeof(uint32_t) + 15u) & ~(size_t)15u;
    p.scan_at = p.total_at + 16u;
    p.scan_bytes = ((size_t)p.n * (RSRT_JPEG_BLOCK_BITS / 32u) + 2u) * sizeof(uint32_t);
    p.bytes = p.scan_at + p.scan_bytes;
    return p;
}

// stages 2 and 3 behind first(scratch), which fills the coefficients and the words, then the file into host_out
template <class First>
rsrt_status jpeg_file(rsrt_context *ctx, const char *what, const JpegPlan &p, const rsrt_jpeg_params *jpeg, First first, void *host_out, size_t capacity, size_t *n_bytes_out)
{
    unsigned long long total = 0ull;
    std::vector<unsigned char> scan;
    const rsrt_status st = read_back_counted(
        ctx, p.bytes,
        [&](void *tmp) {
            char *const base = static_cast<char *>(tmp);
            int16_t *const coefs = reinterpret_cast<int16_t *>(base);
            uint32_t *const words = reinterpret_cast<uint32_t *>(base + p.words_at), *const offsets = reinterpret_cast<uint32_t *>(base + p.offsets_at);
            HIP_TRY(ctx, hipMemsetAsync(base + p.scan_at, 0, p.scan_bytes, ctx->stream));
            const rsrt_status st1 = first(coefs, words);
            if (st1) return st1;
            rt_jpeg_scan_kernel<<<dim3(1), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(words, p.n, jpeg->subsampling, offsets, reinterpret_cast<unsigned long long *>(base + p.total_at));
            rt_jpeg_pack_kernel<<<dim3((p.n + RT_JP_WAVES - 1u) / RT_JP_WAVES), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(coefs, words, offsets, p.n, jpeg->subsampling,
                                                                                                                   reinterpret_cast<uint32_t *>(base + p.scan_at));
            return RSRT_OK;
        },
        p.total_at, &total, sizeof total, p.scan_at, [&]() { return (size_t)((total + 7ull) / 8ull); }, scan);
    if (st) return st;
    const size_t need = rsrt_jpeg_file(scan.data(), total, p.w, p.h, jpeg, static_cast<uint8_t *>(host_out), capacity);
    *n_bytes_out = need;
    if (need > capacity) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "%s: the file is %zu bytes, capacity %zu", what, need, capacity);
    return RSRT_OK;
}

void jpeg_blocks_launch(rsrt_context *ctx, const DisplayChain &c, const JpegPlan &p, const rsrt_jpeg_params *jpeg, int16_t *coefs, uint32_t *words)
{
    if (jpeg->subsampling == RSRT_JPEG_444)
        rt_jpeg_blocks_kernel<RSRT_JPEG_444><<<dim3((p.mw + RT_JP_WAVES - 1u) / RT_JP_WAVES, p.mh), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, jpeg->quality, p.mw, coefs, words);
    else
        rt_jpeg_blocks_kernel<RSRT_JPEG_420><<<dim3(p.mw, p.mh), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(c, jpeg->quality, p.mw, coefs, words);
}

} // namespace

extern "C" {

rsrt_status rsrt_display_jpeg(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local, float bloom_intensity,
                              const rsrt_colour_params *colour, const rsrt_jpeg_params *jpeg, void *host_out, size_t capacity, size_t *n_bytes_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!n_bytes_out) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "display_jpeg: n_bytes_out is NULL");
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "display_jpeg", CHAIN_COLOUR | CHAIN_JPEG, source, sample_total, exposure, local, colour, nullptr, nullptr, bloom_intensity, host_out,
                                         capacity, &c, nullptr, jpeg);
    if (st) return st;
    const JpegPlan p = jpeg_plan((uint32_t)c.w, (uint32_t)c.h, jpeg->subsampling);
    return jpeg_file(ctx, "display_jpeg", p, jpeg, [&](int16_t *coefs, uint32_t *words) { jpeg_blocks_launch(ctx, c, p, jpeg, coefs, words); return RSRT_OK; }, host_out, capacity,
                     n_bytes_out);
}

rsrt_status rsrt_display_jpeg_coefficients(rsrt_context *ctx, uint32_t source, uint32_t sample_total, float exposure, const rsrt_local_params *local, float bloom_intensity,
                                           const rsrt_colour_params *colour, const rsrt_jpeg_params *jpeg, int16_t *host_coefs, size_t n_values)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    DisplayChain c;
    const rsrt_status st = display_chain(ctx, "display_jpeg_coefficients", CHAIN_COLOUR | CHAIN_JPEG | CHAIN_JPEG_COEFS, source, sample_total, exposure, local, colour, nullptr, nullptr,
                                         bloom_intensity, host_coefs, n_values, &c, nullptr, jpeg);
    if (st) return st;
    const JpegPlan p = jpeg_plan((uint32_t)c.w, (uint32_t)c.h, jpeg->subsampling);
    return read_back(ctx, host_coefs, p.words_at, (size_t)p.n * sizeof(uint32_t), [&](void *tmp) {
        jpeg_blocks_launch(ctx, c, p, jpeg, static_cast<int16_t *>(tmp), reinterpret_cast<uint32_t *>(static_cast<char *>(tmp) + p.words_at));
        return RSRT_OK;
    });
}

rsrt_status rsrt_jpeg_encode_coefficients(rsrt_context *ctx, uint32_t width, uint32_t height, const rsrt_jpeg_params *jpeg, const int16_t *host_coefs, size_t n_values,
                                          void *host_out, size_t capacity, size_t *n_bytes_out)
{
    if (!ctx) return RSRT_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    { rsrt_status st0 = whole_frame(ctx, "jpeg_encode_coefficients"); if (st0) return st0; }
    if (!jpeg) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: jpeg is NULL");
    if (!rsrt_jpeg_params_ok(jpeg)) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: want quality in 1 .. 100, subsampling RSRT_JPEG_420 or RSRT_JPEG_444, flags 0, reserved 0");
    if (!rsrt_jpeg_size_ok(width, height, jpeg->subsampling))
        return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: want sides in 1 .. 65535 and a worst case below 2^32 bits, not %u x %u", width, height);
    const JpegPlan p = jpeg_plan(width, height, jpeg->subsampling);
    if (!host_coefs || n_values != (size_t)p.n * 64u) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: expected %zu values", (size_t)p.n * 64u);
    if (!host_out || !n_bytes_out) return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: host_out or n_bytes_out is NULL");
    for (size_t i = 0; i < n_values; i++)
        if (!rsrt_jpeg_value_ok(host_coefs[i], i % 64u == 0u))
            return fail(ctx, RSRT_ERR_INVALID_ARGUMENT, "jpeg_encode_coefficients: value %d at %zu is outside [-1023, 1023] (a DC: [-1024, 1023])", (int)host_coefs[i], i);
    return jpeg_file(ctx, "jpeg_encode_coefficients", p, jpeg, [&](int16_t *coefs, uint32_t *words) {
        HIP_TRY(ctx, hipMemcpyAsync(coefs, host_coefs, p.words_at, hipMemcpyHostToDevice, ctx->stream));
        rt_jpeg_count_kernel<<<dim3((p.n + RT_JP_WAVES - 1u) / RT_JP_WAVES), dim3(RT_LC_BLOCK), 0, ctx->stream>>>(coefs, p.n, jpeg->subsampling, words);
        return RSRT_OK;
    }, host_out, capacity, n_bytes_out);
}

} // extern "C"
