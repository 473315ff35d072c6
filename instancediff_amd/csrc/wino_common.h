// The Winograd toolbox: every definition that the 3x3 Winograd translation units share (conv_wino.hip, conv_wino4.hip, conv_wino4h.hip,
// conv_wino_wgrad.hip, conv_wino4_wgrad.hip; conv1x1_x3.hip takes scalar_ptr).  The packer, the two F(4x4,3x3) forward kernels and the
// F(4x4,3x3) weight gradient must agree on pos() and on the transform matrices: they do because these are the only definitions.
// Device helpers are __forceinline__: a kernel's code is what it was with the helper written out in its own file.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace idiff_detail {
// IDIFF_WINOGRAD=0 (first character '0') turns every Winograd kernel off, forward and weight gradient.  The one reader of the variable
// (conv_wino.hip); IDIFF_WINOGRAD4 and IDIFF_WGRAD4 have their own readers beside the kernels they switch.
bool winograd_disabled();
}  // namespace idiff_detail

namespace idiff_wino {

// ---- device helpers ---------------------------------------------------------------------------------------------------------------

template <int CTRL>
__device__ __forceinline__ float dpp_row_shr(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over each 16-lane row by DPP prefix adds (row_shr 1, 2, 4, 8; zeros shift in): lane 15 of the row ends with the total -- the
// GroupNorm-partials row sum of every forward epilogue
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_row_shr<0x111>(v);
    v += dpp_row_shr<0x112>(v);
    v += dpp_row_shr<0x114>(v);
    v += dpp_row_shr<0x118>(v);
    return v;
}

// A wave-uniform pointer pinned to scalar registers.  Under register pressure the compiler may keep a uniform 64-bit address in
// vector registers; a buffer resource built from it then costs a waterfall loop (readfirstlane + compare + exec masking) around
// EVERY buffer load that uses it.  (Returns T*: what __builtin_amdgcn_make_buffer_rsrc takes.)
template <typename T>
__device__ __forceinline__ T* scalar_ptr(const T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

// ---- F(4x4,3x3): position numbering and transform matrices (interpolation points 0, +-1, +-2, inf) ----------------------------------

// Numbering of the 36 Winograd positions (u, v) into 9 quads of 4: the first four columns of row u fill quad PF(u), its last
// two a half of quad PH(u) shared with the neighbouring row -- every row is one 16-byte and one 8-byte piece at fixed places,
// so the transform writes them without looking at the row's parity.  This numbering IS the layout of the weight image of
// idiff_pack_conv_weight_wino4 (quad-major, four positions per 16-byte A operand) and of every LDS operand image built from it.
__host__ __device__ constexpr int PF(int u) { return (3 * u + 1) / 2; }       // 0, 2, 3, 5, 6, 8
__host__ __device__ constexpr int PH(int u) { return 1 + 3 * (u / 2); }       // 1, 1, 4, 4, 7, 7
__host__ __device__ constexpr int pos(int u, int v) { return v < 4 ? 4 * PF(u) + v : 4 * PH(u) + 2 * (u & 1) + (v - 4); }

// Which positions carry anything when the source is a nearest x2 upsample.  The 6x6 input tile of a 4x4 output tile starts at an odd row
// and column of the x2 grid (oy = y0 - 1 + r with y0 % 4 == 0, source row oy >> 1: gather_decode), so tile rows 1 and 2 are the same
// low-resolution row bit for bit, and so are rows 3 and 4; Hout and Wout are even, so such a pair lies wholly inside the image or is
// wholly padding.  The columns behave the same way.  In B^T d B as the kernels compute it, Winograd row 2 is fma(-1, Y, X) with
// X = fma(-4, d2, d4) and Y = fma(-4, d1, d3) the same bits, and column 2 is p - q of bt6 with p and q the same bits: every position
// (u, v) with u == 2 or v == 2 is exactly +0 in every tile, 11 of the 36, and its accumulator stays the +0 it starts from
// (+0 + (+-0) = +0).  A kernel that leaves those products out and hands literal +0 to the output transform returns the bits of one that
// multiplies all 36 (finite operands: 0 * inf is NaN only where the product is formed).  tests/test_wino_upsample_cpu.py checks the rule
// by brute force over every tile of padded images, border tiles included: these 11 are always zero and none of the other 25 is.
template <bool UPSAMPLED>
__host__ __device__ constexpr bool pos_live(int u, int v) {
    return !UPSAMPLED || (u != 2 && v != 2);
}
// the same per position quad of pos(): bit c = component c of the quad's 16-byte operands is live (normal source: 0xf throughout;
// upsampled: quads 0, 2, 5, 6, 8 -> {0, 1, 3}, quads 1, 7 -> all four, quad 4 -> {2, 3}, quad 3 -> none)
template <bool UPSAMPLED>
__host__ __device__ constexpr unsigned quad_live(int quad) {
    unsigned m = 0;
    for (int u = 0; u < 6; ++u)
        for (int v = 0; v < 6; ++v)
            if (pos_live<UPSAMPLED>(u, v) && pos(u, v) / 4 == quad) m |= 1u << (pos(u, v) & 3);
    return m;
}

// one 6-point input transform B^T x.  UPSAMPLED (pos_live): o[2] is exactly +0 and no reader takes it; it is left holding p, which is
// at hand, instead of spending the subtraction
template <bool UPSAMPLED = false>
__device__ __forceinline__ void bt6(const float (&x)[6], float (&o)[6]) {
    o[0] = __builtin_fmaf(4.f, x[0], __builtin_fmaf(-5.f, x[2], x[4]));
    const float p = __builtin_fmaf(-4.f, x[2], x[4]), q = __builtin_fmaf(-4.f, x[1], x[3]);
    o[1] = p + q;
    o[2] = UPSAMPLED ? p : p - q;
    const float c = x[4] - x[2], e = x[3] - x[1];
    o[3] = __builtin_fmaf(2.f, e, c);
    o[4] = __builtin_fmaf(-2.f, e, c);
    o[5] = __builtin_fmaf(4.f, x[1], __builtin_fmaf(-5.f, x[3], x[5]));
}
// one 6 -> 4 output transform A^T x
__device__ __forceinline__ void at6(const float x0, const float x1, const float x2, const float x3, const float x4, const float x5, float (&o)[4]) {
    const float s1 = x1 + x2, d1 = x1 - x2, s2 = x3 + x4, d2 = x3 - x4;
    o[0] = (x0 + s1) + s2;
    o[1] = __builtin_fmaf(2.f, d2, d1);
    o[2] = __builtin_fmaf(4.f, s2, s1);
    o[3] = __builtin_fmaf(8.f, d2, d1) + x5;
}
// A x for a 4-point x (the weight gradient's dY transform): the six rows of A = [1 0 0 0; 1 1 1 1; 1 -1 1 -1; 1 2 4 8; 1 -2 4 -8; 0 0 0 1]
__device__ __forceinline__ void a6(float x0, float x1, float x2, float x3, float (&o)[6]) {
    const float s = x0 + x2, t = x1 + x3;
    o[0] = x0;
    o[1] = s + t;
    o[2] = s - t;
    const float p = __builtin_fmaf(4.f, x2, x0), q = __builtin_fmaf(8.f, x3, 2.f * x1);
    o[3] = p + q;
    o[4] = p - q;
    o[5] = x3;
}
// G x for a 3-point x (the packer's weight transform): G rows [1/4,0,0], [-1/6,-1/6,-1/6], [-1/6,1/6,-1/6], [1/24,1/12,1/6], [1/24,-1/12,1/6], [0,0,1]
__device__ __forceinline__ void g6(float x0, float x1, float x2, float (&o)[6]) {
    o[0] = 0.25f * x0;
    const float s = x0 + x2;
    o[1] = (-1.f / 6.f) * (s + x1);
    o[2] = (-1.f / 6.f) * (s - x1);
    const float t = __builtin_fmaf(4.f, x2, x0);  // x0 + 4 x2
    o[3] = (1.f / 24.f) * __builtin_fmaf(2.f, x1, t);
    o[4] = (1.f / 24.f) * __builtin_fmaf(-2.f, x1, t);
    o[5] = x2;
}
// G^T m for a 6-point m (the weight gradient's output transform): sum_u G[u][p] m[u]
__device__ __forceinline__ void gt3(float m0, float m1, float m2, float m3, float m4, float m5, float (&o)[3]) {
    const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
    o[0] = __builtin_fmaf(0.25f, m0, __builtin_fmaf(-1.f / 6.f, s12, (1.f / 24.f) * s34));
    o[1] = __builtin_fmaf(-1.f / 6.f, d12, (1.f / 12.f) * d34);
    o[2] = __builtin_fmaf(-1.f / 6.f, s12, __builtin_fmaf(1.f / 6.f, s34, m5));
}

// ---- the gather table of one F(4x4,3x3) item ----------------------------------------------------------------------------------------
// Thread `tid` stages R[tid + i*NT], i < NL: the R index itself enumerates (ci, row, col) with channel stride PSP (PS used) and row
// stride RS (RCOLS used).  An element's load offset (bytes inside the sample) is -1 for pad slots and for elements outside the image:
// the buffer load's range check fails and it reads 0.0.  Writes gtab[i * NT + tid] (thread-private entries) for the patch whose first
// output pixel is (y0, x0) of the conv `a` (Hout, Wout, Win) and sets the padding mask `om` (bit i: element i is padding / outside).
// Every argument is a reference and is read where the kernels' own copies of this loop read it: by value, or with the mask as the
// return value, the F(4x4,3x3) forward kernels' instruction order and register assignment change.
template <int MODE, int NT, int NL, int PSP, int PS, int RS, int RCOLS, typename Args>
__device__ __forceinline__ void gather_decode(const int& tid, unsigned& om, const int& y0, const int& x0, const Args& a, int* const& gtab, const int& HWin) {
    int t = tid;
    asm volatile("" : "+v"(t));  // opaque: keeps the decode here, once per item, instead of hoisted out of the item loop and held in registers
    om = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int e = t + i * NT;
        const int ci = e / PSP;
        const int rem = e - ci * PSP;
        const int r = rem / RS;
        const int c = rem - r * RS;
        const int oy = y0 - 1 + r, ox = x0 - 1 + c;  // output-grid coordinates of the element
        const bool in = rem < PS && c < RCOLS && (unsigned)oy < (unsigned)a.Hout && (unsigned)ox < (unsigned)a.Wout;
        const int sp = MODE == IDIFF_CONV_UPSAMPLE2 ? (oy >> 1) * a.Win + (ox >> 1) : oy * a.Win + ox;
        gtab[i * NT + tid] = in ? (ci * HWin + sp) * 4 : -1;
        om |= (in ? 0u : 1u) << i;
    }
}

// The same table in 16-byte pieces (normal mode, Win % 4 == 0, x0 % 4 == 0, 16-byte aligned sources and batch strides of whole
// float4): R is counted in float4 slots -- channel stride PSP4 (PS4 used), RS4 slots per row -- and its column origin lies three floats
// to the left: row float 3 + c holds patch column c, so that slot j of a row is the ALIGNED global piece ox = x0 - 4 + 4j .. x0 - 1 + 4j,
// wholly inside the image or wholly outside (Wout % 4 == 0).  Thread `tid` stages slots e0 + i*ES, i < NR (the kernel deals whole
// wave-instructions of 64 slots to its waves: e0 and NR are the caller's); gtab[i * NT + tid] and the mask (bit i: the thread's slot i
// is padding / outside) as above.
template <int NT, int NR, int ES, int PSP4, int PS4, int RS4, typename Args>
__device__ __forceinline__ void gather_decode16(const int& tid, const int& e0, unsigned& om, const int& y0, const int& x0, const Args& a, int* const& gtab, const int& HWin) {
    int t = e0;
    asm volatile("" : "+v"(t));  // (as above)
    om = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int e = t + i * ES;
        const int ci = e / PSP4;
        const int rem = e - ci * PSP4;
        const int r = rem / RS4;
        const int j = rem - r * RS4;
        const int oy = y0 - 1 + r, ox4 = x0 - 4 + 4 * j;  // the row and the first column of the piece
        const bool in = rem < PS4 && (unsigned)oy < (unsigned)a.Hout && (unsigned)ox4 < (unsigned)a.Wout;
        gtab[i * NT + tid] = in ? (ci * HWin + oy * a.Win + ox4) * 4 : -1;
        om |= (in ? 0u : 1u) << i;
    }
}

// ---- the 3x3 weight as the packers read it --------------------------------------------------------------------------------------------
// taps of (co, ci) of the conv the kernel runs: w[co][ci] as stored, or -- transpose: the input-gradient conv -- w[ci][co] rotated by 180
// degrees (Cin = the stored tensor's second dimension)
__device__ __forceinline__ void load_taps(const float* __restrict__ w, int Cin, int co, int ci, int transpose, float (&g)[3][3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            g[p][q] = transpose ? w[((long long)ci * Cin + co) * 9 + (2 - p) * 3 + (2 - q)] : w[((long long)co * Cin + ci) * 9 + p * 3 + q];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------

// Body of an idiff_pack_conv_weight_wino* entry: NPOS Winograd positions per (co, ci) pair, `kern` one of the pack kernels.
template <int NPOS, typename K>
int pack_entry(const char* name, K kern, const float* w, float* image, int Cout, int Cin, int transpose, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(w && image && Cout > 0 && Cin > 0, "%s: bad args", name);
    const int Co = transpose ? Cin : Cout, Ci = transpose ? Cout : Cin;
    IDIFF_CHECK_ARG(Co % 16 == 0 && Ci % 8 == 0, "%s: needs conv Cout %% 16 == 0 and Cin %% 8 == 0 (got %d, %d)", name, Co, Ci);
    if (Co % 64) {  // partial last 64-channel block: its unused rows must read as zero
        hipError_t e = hipMemsetAsync(image, 0, (size_t)NPOS * Ci * ((Co + 63) / 64) * 64 * sizeof(float), (hipStream_t)stream);
        if (e != hipSuccess) IDIFF_FAIL(IDIFF_E_HIP, "%s: hipMemsetAsync: %s", name, hipGetErrorString(e));
    }
    const long long n = (long long)Cout * Cin;
    const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, image, Cout, Cin, transpose);
    IDIFF_CHECK_LAUNCH(name);
    return IDIFF_OK;
}

// Persistent grid: `slots` workgroups fit the device at once; every workgroup walks `per` items (the last one maybe fewer), none is empty.
inline int persistent_grid(int total, int slots, int* per_out = nullptr) {
    const int per = (total + slots - 1) / slots;
    if (per_out) *per_out = per;
    return (total + per - 1) / per;
}

// The forward kernels' instantiation ladder: (mode, prologue, second source, ragged image) -> launch(<MODE>, <SPEC>, <RAG>) with
// SPEC 1 = single source, no prologue; 2 = single source + GN/FiLM/SiLU prologue; 3 = two sources (virtual concat).  The eligibility
// checks have excluded upsample with a prologue or a second source, and a prologue together with a second source.
template <typename F>
int launch_spec_ladder(int mode, bool pro, bool src1, bool ragged, F&& launch) {
    auto rag = [&](auto mode_tag, auto spec_tag) {
        if (ragged) return launch(mode_tag, spec_tag, std::true_type{});
        return launch(mode_tag, spec_tag, std::false_type{});
    };
    using Normal = std::integral_constant<int, IDIFF_CONV_NORMAL>;
    using Upsample = std::integral_constant<int, IDIFF_CONV_UPSAMPLE2>;
    if (mode == IDIFF_CONV_UPSAMPLE2) return rag(Upsample{}, std::integral_constant<int, 1>{});
    if (pro) return rag(Normal{}, std::integral_constant<int, 2>{});
    if (src1) return rag(Normal{}, std::integral_constant<int, 3>{});
    return rag(Normal{}, std::integral_constant<int, 1>{});
}

}  // namespace idiff_wino

// ---- -DIDIFF_WINO_TRACE (debug builds; compiled out of the product): per-phase cycle counts summed over all items, printed by the
// launcher.  N = number of phases: TRACE_MARK(k), k = 0..N, closes phase k-1; TRACE_LAP(last) at an item's top adds the time since the
// previous item's mark `last` to phase `last`.
#ifdef IDIFF_WINO_TRACE
#define TRACE_PARAM , long long* trace
#define TRACE_INIT(N) long long tr_t[(N) + 1] = {0}, tr_acc[N] = {0};
#define TRACE_MARK(k)                       \
    tr_t[k] = __builtin_readcyclecounter(); \
    if (k > 0) tr_acc[k - 1] += tr_t[k] - tr_t[k - 1];
#define TRACE_LAP(last) \
    if (tr_t[last] != 0) tr_acc[last] += tr_t[0] - tr_t[last];
#define TRACE_FINI(N)                                                                                                   \
    if (tid == 0) {                                                                                                     \
        for (int q_ = 0; q_ < (N); ++q_) atomicAdd((unsigned long long*)trace + q_, (unsigned long long)tr_acc[q_]);    \
    }
#else
#define TRACE_PARAM
#define TRACE_INIT(N)
#define TRACE_MARK(k)
#define TRACE_LAP(last)
#define TRACE_FINI(N)
#endif
