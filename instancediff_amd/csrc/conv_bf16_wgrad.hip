// Weight gradient of the bf16-operand 3x3 conv (conv_bf16.hip; idiff_conv_desc.operands == 1): gfx950, v_mfma_f32_16x16x32_bf16.
//
//   dW[co][ci][ky][kx] = sum_{b,y,x} bf16(dY[b,co,y,x]) * bf16(X~[b,ci,y+ky-1,x+kx-1]), summed in fp32, where X~ is re-gathered exactly
//   as the forward gathers it (virtual concat, nearest x2 upsample, prologue affine + SiLU, then zero padding) and rounded once
//   (plain cast, round to nearest even).
//
//   GEMM view per workgroup: M = 64 output channels, N = 32 input channels x 9 taps, K = the pixels of one K-block: up to 16 8x32
//   patches (4096 pixels) of ONE sample.  Wave w owns channels 16w .. 16w+15 x 32 ci x 9 taps (18 accumulators of 16x16).  Per patch,
//   dY is staged in LDS as [co][256 px] bf16 and X~ as three column-shifted copies [kx][ci][10 rows][32 px] bf16, so that every
//   operand fragment (eight consecutive pixels of one row) is one aligned ds_read_b128 for every tap.
//
//   Determinism: each K-block writes its own partial [kb][co][ci][3][3]; the reduction adds the partials in K-block order (sample 0's
//   blocks first), one thread per weight, no atomics.  The K-blocks are fixed by the per-sample shape alone, so the result does not
//   depend on the grid, and with one K-block per sample (<= 4096 output pixels) dW(B) is exactly the fp32 sum, in sample order, of
//   the single-sample gradients.
#include "conv_wgrad_args.h"

namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 64, BN = 32, TH = 8, TW = 32, HR = TH + 2, G = 16;
constexpr int YST = TH * TW * 2 + 16;     // 528: dY row pitch (bytes)
constexpr int XST = HR * TW * 2 + 16;     // 656: X~ channel pitch (bytes)
constexpr int XCOPY = BN * XST;           // 20992: one column-shifted copy
constexpr int Y_BYTES = BM * YST;         // 33792
constexpr int X_BYTES = 3 * XCOPY;        // 62976
constexpr int NYI = BM * TH * TW / 8 / 256;  // 8 dY items (eight pixels) per thread
constexpr int NXI = 3 * BN * HR * 4 / 256;   // 15 X~ items per thread
static_assert(3 * BN * HR * 4 % 256 == 0, "X~ items");

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};  // v_cvt_pk_bf16_f32: round to nearest even
    return __builtin_bit_cast(unsigned, v);
}

__device__ __forceinline__ floatx4 mma(const uintx4& a, const uintx4& b, const floatx4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

struct Geo {
    int tiles_x, ntiles, nkbs, ncob, ncib;
};

inline Geo geometry(int Cin, int Cout, int Hout, int Wout) {
    Geo g;
    g.tiles_x = Wout / TW;
    g.ntiles = g.tiles_x * (Hout / TH);
    g.nkbs = (g.ntiles + G - 1) / G;
    g.ncob = Cout / BM;
    g.ncib = Cin / BN;
    return g;
}

template <int MODE>
__global__ __launch_bounds__(256, 1) void wgrad_bf16_kernel(const idiff_detail::WwArgs a, const Geo geo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const Ys = smem;
    unsigned char* const Xs = smem + Y_BYTES;
    float* const protab = reinterpret_cast<float*>(smem + Y_BYTES + X_BYTES);  // [2][32] prologue affine of this ci block

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n16 = lane & 15, kgl = lane >> 4;

    int id = blockIdx.x;
    const int cib = id % geo.ncib;
    id /= geo.ncib;
    const int cob = id % geo.ncob;
    id /= geo.ncob;
    const int g = id % geo.nkbs;
    const int b = id / geo.nkbs;
    const int co0 = cob * BM, ci0 = cib * BN;
    const bool has_pro = a.pro_a != nullptr;
    const long long HWin = (long long)a.Hin * a.Win, HWo = (long long)a.Hout * a.Wout;
    const float* const xsrc = ci0 >= a.C0v ? a.src1 + (long long)b * a.bs1 + (long long)(ci0 - a.C0v) * HWin
                                           : a.src0 + (long long)b * a.bs0 + (long long)ci0 * HWin;
    const float* const dyb = a.dy + (long long)b * a.dybs + (long long)co0 * HWo;
    if (has_pro && tid < BN) {
        protab[tid] = a.pro_a[(long long)b * a.C0r + ci0 + tid];
        protab[BN + tid] = a.pro_b[(long long)b * a.C0r + ci0 + tid];
    }

    floatx4 acc[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[t][n] = floatx4{0.f, 0.f, 0.f, 0.f};

    const unsigned char* const ard = Ys + (16 * wave + n16) * YST + kgl * 16;
    const unsigned char* const brd = Xs + n16 * XST + kgl * 16;
    const int t_end = min((g + 1) * G, geo.ntiles);
    for (int t = g * G; t < t_end; ++t) {
        const int y0 = (t / geo.tiles_x) * TH, x0 = (t % geo.tiles_x) * TW;
        __syncthreads();  // the previous patch's operands are consumed (and protab is visible)
#pragma unroll
        for (int i = 0; i < NYI; ++i) {  // item = (co, row, octet of 8 pixels), octet fastest
            const int e = tid + i * 256;
            const int po = e & 3, row = (e >> 2) & 7, co = e >> 5;
            const float* const p = dyb + (long long)co * HWo + (long long)(y0 + row) * a.Wout + x0 + 8 * po;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p[j];
            const uintx4 pk = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
            *reinterpret_cast<uintx4*>(Ys + co * YST + (row * TW + 8 * po) * 2) = pk;
        }
#pragma unroll 3
        for (int i = 0; i < NXI; ++i) {  // item = (kx, ci, halo row, octet), octet fastest
            const int e = tid + i * 256;
            const int po = e & 3, hr = (e >> 2) % HR, r2 = (e >> 2) / HR;
            const int ci = r2 % BN, kx = r2 / BN;
            const int oy = y0 - 1 + hr;
            const float* const pc = xsrc + (long long)ci * HWin;
            const bool rowv = oy >= 0 && oy < a.Hout;
            const float pa = has_pro ? protab[ci] : 0.f, pb = has_pro ? protab[BN + ci] : 0.f;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ox = x0 - 1 + kx + 8 * po + j;
                const bool ok = rowv && ox >= 0 && ox < a.Wout;
                const int off = MODE == IDIFF_CONV_UPSAMPLE2 ? (oy >> 1) * a.Win + (ox >> 1) : oy * a.Win + ox;
                float x = pc[ok ? off : 0];
                if (has_pro) x = silu_fast(pa * x + pb);
                v[j] = ok ? x : 0.f;  // zero padding after the activation
            }
            const uintx4 pk = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
            *reinterpret_cast<uintx4*>(Xs + kx * XCOPY + ci * XST + (hr * TW + 8 * po) * 2) = pk;
        }
        __syncthreads();
        for (int r = 0; r < TH; ++r) {  // K-step: the 32 pixels of patch row r
            const uintx4 af = *reinterpret_cast<const uintx4*>(ard + r * TW * 2);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const uintx4 bfr = *reinterpret_cast<const uintx4*>(brd + kx * XCOPY + n * 16 * XST + (r + ky) * TW * 2);
                    acc[tap][n] = mma(af, bfr, acc[tap][n]);
                }
            }
        }
    }
    // partial of this K-block in torch layout: lane holds ci 16 n + n16, co 16 wave + 4 kgl + rr
    const long long nw = 9ll * a.Cin * a.Cout;
    float* const wsb = a.ws + ((long long)b * geo.nkbs + g) * nw;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int co = co0 + 16 * wave + 4 * kgl + rr, ci = ci0 + 16 * n + n16;
                wsb[((long long)co * a.Cin + ci) * 9 + tap] = acc[tap][n][rr];
            }
}

// dw[i] (+)= sum over K-blocks, in order, of ws[kb][i]
__global__ __launch_bounds__(256) void wgrad_bf16_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int nkb, long long n, int accumulate) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float t = 0.f;
        for (int k = 0; k < nkb; ++k) t += ws[(long long)k * n + i];
        dw[i] = accumulate ? dw[i] + t : t;
    }
}

}  // namespace

namespace idiff_detail {

bool bf16_wgrad_eligible(const WwArgs& a, int ks, int mode) {
    return ks == 3 && (mode == IDIFF_CONV_NORMAL || mode == IDIFF_CONV_UPSAMPLE2) && a.Cout % BM == 0 && a.C0v % BN == 0 && a.C1v % BN == 0 &&
           a.Cin >= BN && a.Hout % TH == 0 && a.Wout % TW == 0 && (long long)a.Hout * a.Wout < (1ll << 30);
}

long long bf16_wgrad_ws_floats(int Cin, int Cout, int B, int Hout, int Wout) {
    const Geo g = geometry(Cin, Cout, Hout, Wout);
    return (long long)B * g.nkbs * 9 * Cin * Cout;
}

int launch_bf16_wgrad(const WwArgs& a, float* dw, int accumulate, hipStream_t st) {
    const Geo g = geometry(a.Cin, a.Cout, a.Hout, a.Wout);
    const long long nwg = (long long)a.B * g.nkbs * g.ncob * g.ncib;
    IDIFF_CHECK_ARG(nwg < (1ll << 31), "conv2d_wgrad(bf16): grid too large");
    const size_t lds = Y_BYTES + X_BYTES + 2 * BN * sizeof(float);
    static idiff_dyn_lds_cache lds_cache[2];
    const bool ups = a.ups != 0;
    auto kern = ups ? wgrad_bf16_kernel<IDIFF_CONV_UPSAMPLE2> : wgrad_bf16_kernel<IDIFF_CONV_NORMAL>;
    if (const int rc = idiff_dyn_lds(lds_cache[ups], kern, lds, "conv2d_wgrad(bf16)")) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(256), lds, st, a, g);
    IDIFF_CHECK_LAUNCH("conv2d_wgrad(bf16)");
    const long long n = 9ll * a.Cin * a.Cout;
    const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
    hipLaunchKernelGGL(wgrad_bf16_reduce_kernel, dim3(grid), dim3(256), 0, st, a.ws, dw, (int)(a.B * g.nkbs), n, accumulate);
    IDIFF_CHECK_LAUNCH("conv2d_wgrad_reduce(bf16)");
    return IDIFF_OK;
}

}  // namespace idiff_detail
