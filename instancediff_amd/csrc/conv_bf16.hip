// 3x3 convolution on the bf16 matrix cores with bf16-ROUNDED operands (gfx950, v_mfma_f32_16x16x32_bf16) -- the opt-in
// reduced-precision variant (idiff_conv_desc.operands == 1, IDIFF_CONV_ALGO_BF16).  Not the default path.
//
//   Numerics contract: every gathered input operand is first computed in fp32 exactly as conv_igemm.hip computes it (virtual concat
//   of two sources, nearest x2 upsample, the GroupNorm/FiLM affine + SiLU prologue, then zero padding); each operand and each weight
//   is then rounded ONCE to bf16, round-to-nearest-even (a plain cast: v_cvt_pk_bf16_f32, which keeps NaNs).  The products are
//   summed in fp32 on the matrix cores.  Everything after the sum is the fp32 epilogue of conv_igemm.hip: bias, GroupNorm partials
//   of acc + bias in the [B][idiff_conv2d_num_tiles][Cout][2] layout, per-(b,c) vector, residual, "+ silu(a*aux+b)".
//
//   GEMM view: M = 64 output channels, N = 256 pixels (an 8x32 patch of one sample, the GroupNorm-partials tile of the other 3x3
//   kernels), K = 9 taps x Cin, walked in chunks of 32 input channels.  256 threads; wave w owns patch rows 2w, 2w+1 (64 pixels) x
//   all 64 channels = 4x4 accumulator blocks of 16x16.  Per chunk the 10x34-pixel halo of 32 channels is gathered in fp32, activated,
//   rounded and written to LDS as [channel octet][halo pixel][8 bf16] (one ds_write_b128 per pixel and octet: the eight channels of a
//   pixel are exactly the K-octet a lane of the B operand holds); the chunk's weights come pre-rounded in the kernel's fragment order
//   (idiff_pack_conv_weight_bf16) and are copied verbatim.  Single LDS buffer (58 KB + tables: two workgroups per CU); the global
//   loads of chunk c+1 are in flight in registers while the 144 MFMAs per wave of chunk c run.
//
//   Eligible (conv_bf16_eligible): ks == 3, NORMAL or UPSAMPLE2, Cout % 64 == 0, C0 % 32 == 0 and C1 % 32 == 0 (a chunk lies in one
//   source), Hout % 8 == 0, Wout % 32 == 0.  Roofline: 2.5 PFLOP/s dense bf16 (4x the multiply-adds of F(4x4,3x3), 16x the rate).
#include "conv_args.h"

using idiff_detail::ConvArgs;

namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 64, CK = 32, TH = 8, TW = 32, HR = TH + 2, HC = TW + 2, HP = HR * HC;  // 340 halo pixels
constexpr int XSLOT = 352;                 // halo-pixel slots per octet plane: a multiple of 16, so the 16 lanes of each ds_read_b128
                                           // lane group (4 + 4 consecutive pixels of octet k, 8 of octet k+1) hit 16 distinct bank quads
constexpr int X_BYTES = 4 * XSLOT * 16;    // 22528
constexpr int W_BYTES = 9 * 4 * BM * 16;   // 36864: one (chunk, 64-channel block) of the weight image
constexpr int NXI = (4 * HP + 255) / 256;  // 6 staging items (pixel, octet) per thread
constexpr int NWI = W_BYTES / 16 / 256;    // 9 weight pieces of 16 bytes per thread
constexpr int FIXED_LDS = X_BYTES + W_BYTES + (4 * BM + 4 * BM * 2) * 4;

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};  // round to nearest even, NaN stays NaN (v_cvt_pk_bf16_f32)
    return __builtin_bit_cast(unsigned, v);
}

__device__ __forceinline__ floatx4 mma(const uintx4& a, const uintx4& b, const floatx4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void conv_bf16_kernel(const ConvArgs a, const uintx4* __restrict__ wimg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const Xs = smem;
    unsigned char* const Ws = smem + X_BYTES;
    float* const econst = reinterpret_cast<float*>(smem + X_BYTES + W_BYTES);  // [4][64] bias, vec, aux_a, aux_b
    float* const red = econst + 4 * BM;                                          // [4 waves][64][2] GroupNorm partials
    float* const protab = red + 4 * BM * 2;                                      // [2][C0r] prologue affine of this sample

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n16 = lane & 15, kgl = lane >> 4;

    const unsigned logical = xcd_remap(blockIdx.x, a.total_wg);
    const int cob = logical % a.ncob;
    const int tile = (logical / a.ncob) % a.ntiles;
    const int b = logical / (a.ncob * a.ntiles);
    const int co0 = cob * BM;
    const int y0 = (tile / a.tiles_x) * TH;
    const int x0 = (tile % a.tiles_x) * TW;
    const bool has_pro = a.pro_a != nullptr;
    const long long HWin = (long long)a.Hin * a.Win;

    if (has_pro) {
        for (int i = tid; i < a.C0r; i += 256) {
            protab[i] = a.pro_a[(long long)b * a.C0r + i];
            protab[a.C0r + i] = a.pro_b[(long long)b * a.C0r + i];
        }
    }
    {
        const int which = tid / BM, co = co0 + tid % BM;  // Cout % 64 == 0: every channel of the block exists
        float v = 0.f;
        if (which == 0 && a.bias) v = a.bias[co];
        if (which == 1 && a.vec) v = a.vec[(long long)b * a.Cout + co];
        if (which == 2 && a.aux) v = a.aux_a[(long long)b * a.Cout + co];
        if (which == 3 && a.aux) v = a.aux_b[(long long)b * a.Cout + co];
        econst[tid] = v;
    }

    // ---- staging: item e = (octet, halo pixel), pixel fastest (lanes read consecutive pixels of one channel) -----------------------
    int goff[NXI], goct[NXI];
    bool gval[NXI];
#pragma unroll
    for (int i = 0; i < NXI; ++i) {
        const int e = tid + i * 256;
        const int oct = min(e / HP, 3);
        const int hp = e - oct * HP;
        const int hr = hp / HC, hc = hp - hr * HC;
        const int oy = y0 - 1 + hr, ox = x0 - 1 + hc;
        const bool v = e < 4 * HP && oy >= 0 && oy < a.Hout && ox >= 0 && ox < a.Wout;
        const int off = MODE == IDIFF_CONV_UPSAMPLE2 ? (oy >> 1) * a.Win + (ox >> 1) : oy * a.Win + ox;
        goff[i] = v ? off : 0;
        gval[i] = v;
        goct[i] = oct;
    }
    float xr[NXI][8];
    uintx4 wr[NWI];
    const int nchunks = a.Cin / CK;

    auto load = [&](int cc) {
        const int cb = cc * CK;  // uniform; a chunk lies in one source
        const float* const base = cb >= a.C0v ? a.src1 + (long long)b * a.bs1 + (long long)(cb - a.C0v) * HWin
                                              : a.src0 + (long long)b * a.bs0 + (long long)cb * HWin;
#pragma unroll
        for (int i = 0; i < NXI; ++i) {
            const float* const p = base + (long long)goct[i] * 8 * HWin + goff[i];  // masked items read a valid element, zeroed below
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[i][j] = p[j * HWin];
        }
        const uintx4* const wsrc = wimg + ((long long)cc * a.ncob + cob) * (W_BYTES / 16);
#pragma unroll
        for (int i = 0; i < NWI; ++i) wr[i] = wsrc[tid + i * 256];
    };
    auto write = [&](int cc) {
        const int cb = cc * CK;
#pragma unroll
        for (int i = 0; i < NXI; ++i) {
            const int e = tid + i * 256;
            if (e < 4 * HP) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float x = xr[i][j];
                    if (has_pro) {  // single source: channel cb + 8 oct + j < C0r
                        const int ch = cb + goct[i] * 8 + j;
                        x = silu_fast(protab[ch] * x + protab[a.C0r + ch]);
                    }
                    v[j] = gval[i] ? x : 0.f;  // zero padding after the activation
                }
                const uintx4 pk = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
                const int hp = e - goct[i] * HP;
                *reinterpret_cast<uintx4*>(Xs + (goct[i] * XSLOT + hp) * 16) = pk;
            }
        }
#pragma unroll
        for (int i = 0; i < NWI; ++i) reinterpret_cast<uintx4*>(Ws)[tid + i * 256] = wr[i];
    };

    floatx4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[mi][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // A operand (weights): lane holds co 16 mi + n16, ci 8 kgl .. 8 kgl + 7 of a tap; B operand (pixels): lane holds pixel n16 of block
    // j (patch row 2 wave + j / 2, columns 16 (j & 1) ..), the same eight channels
    const unsigned char* const wrd = Ws + (kgl * BM + n16) * 16;
    const unsigned char* const xrd = Xs + (kgl * XSLOT + 2 * wave * HC + n16) * 16;

    load(0);
    __syncthreads();  // protab visible
    write(0);
    __syncthreads();
    for (int cc = 0; cc < nchunks; ++cc) {
        if (cc + 1 < nchunks) load(cc + 1);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            uintx4 af[4], bf[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) af[mi] = *reinterpret_cast<const uintx4*>(wrd + tap * (4 * BM * 16) + mi * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const uintx4*>(xrd + (((j >> 1) + ky) * HC + 16 * (j & 1) + kx) * 16);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[mi][j] = mma(af[mi], bf[j], acc[mi][j]);
        }
        if (cc + 1 < nchunks) {
            __syncthreads();  // every wave is done reading chunk cc
            write(cc + 1);
            __syncthreads();
        }
    }

    // ---- epilogue (fp32): lane holds pixel n16 of block j, channels 16 mi + 4 kgl + r --------------------------------------------
    const int HWo = a.Hout * a.Wout;
    float* const outb = a.out + (long long)b * a.obs;
    const float* const resb = a.res ? a.res + (long long)b * a.rbs : nullptr;
    const float* const auxb = a.aux ? a.aux + (long long)b * a.abs_ : nullptr;
    float s[4][4], q[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * mi + 4 * kgl + r;
            const float bv = econst[col], add = econst[BM + col], aa = econst[2 * BM + col], ab = econst[3 * BM + col];
            float* const orow = outb + (long long)(co0 + col) * HWo;
            float ss = 0.f, qq = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int oy = y0 + 2 * wave + (j >> 1), ox = x0 + 16 * (j & 1) + n16;
                const long long o = (long long)(co0 + col) * HWo + oy * a.Wout + ox;
                float v = acc[mi][j][r] + bv;
                ss += v;
                qq += v * v;
                v += add;
                if (resb) v += resb[o];
                if (auxb) v += silu_fast(aa * auxb[o] + ab);
                orow[oy * a.Wout + ox] = v;
            }
            s[mi][r] = ss;
            q[mi][r] = qq;
        }
    if (a.stats) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {  // over the 16 pixels of the lane group, fixed order
                    s[mi][r] += __shfl_xor(s[mi][r], m, 64);
                    q[mi][r] += __shfl_xor(q[mi][r], m, 64);
                }
                if (n16 == 0) {
                    const int col = 16 * mi + 4 * kgl + r;
                    red[(wave * BM + col) * 2 + 0] = s[mi][r];
                    red[(wave * BM + col) * 2 + 1] = q[mi][r];
                }
            }
        __syncthreads();
        if (tid < BM * 2) {
            const int col = tid >> 1, w = tid & 1;
            const float t = red[(0 * BM + col) * 2 + w] + red[(1 * BM + col) * 2 + w] + red[(2 * BM + col) * 2 + w] + red[(3 * BM + col) * 2 + w];
            a.stats[(((long long)b * a.ntiles + tile) * a.Cout + co0 + col) * 2 + w] = t;
        }
    }
}

// image element i (bf16) = [chunk of 32 ci][block of 64 co][tap][octet of 8 ci][co][8]; zero beyond the conv's Cin / Cout
__global__ void pack_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int CoutW, int CinW, int transpose, int ncob, long long n) {
    const int Cc = transpose ? CinW : CoutW, Kc = transpose ? CoutW : CinW;  // the conv's Cout / Cin
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), co = (int)((i >> 3) & 63), oct = (int)((i >> 9) & 3);
        const long long rest = i >> 11;
        const int tap = (int)(rest % 9);
        const long long blk = rest / 9;
        const int cob = (int)(blk % ncob), ck = (int)(blk / ncob);
        const int ci = ck * CK + oct * 8 + j, coa = cob * BM + co;
        float v = 0.f;
        if (ci < Kc && coa < Cc) v = transpose ? w[((long long)ci * CinW + coa) * 9 + (8 - tap)] : w[((long long)coa * CinW + ci) * 9 + tap];
        out[i] = (__bf16)v;
    }
}

}  // namespace

namespace idiff_detail {

bool conv_bf16_eligible(const ConvArgs& a, int ks, int mode, const void* wbf16) {
    return ks == 3 && (mode == IDIFF_CONV_NORMAL || mode == IDIFF_CONV_UPSAMPLE2) && wbf16 != nullptr && (reinterpret_cast<uintptr_t>(wbf16) & 15) == 0 &&
           a.Cout % BM == 0 && a.C0v % CK == 0 && a.C1v % CK == 0 && a.Cin >= CK && a.Hout % TH == 0 && a.Wout % TW == 0 && a.C0r <= 4096 &&
           (long long)a.Hout * a.Wout < (1ll << 30);
}

// `a` carries conv_igemm.hip's 8x32-patch x 64-channel geometry (tiles_x, ntiles, ncob, total_wg) -- the same grid
int launch_conv_bf16(const ConvArgs& a, int mode, const void* wbf16, hipStream_t st) {
    const size_t lds = FIXED_LDS + (a.pro_a ? (size_t)2 * a.C0r * sizeof(float) : 0);
    static idiff_dyn_lds_cache lds_cache[2];
    auto kern = mode == IDIFF_CONV_UPSAMPLE2 ? conv_bf16_kernel<IDIFF_CONV_UPSAMPLE2> : conv_bf16_kernel<IDIFF_CONV_NORMAL>;
    if (const int rc = idiff_dyn_lds(lds_cache[mode == IDIFF_CONV_UPSAMPLE2], kern, lds, "conv2d(bf16)")) return rc;
    hipLaunchKernelGGL(kern, dim3(a.total_wg), dim3(256), lds, st, a, static_cast<const uintx4*>(wbf16));
    IDIFF_CHECK_LAUNCH("conv2d_fwd(bf16)");
    return IDIFF_OK;
}

}  // namespace idiff_detail

extern "C" long long idiff_conv_weight_bf16_bytes(int Cout, int Cin, int transpose) {
    if (Cout <= 0 || Cin <= 0) return -1;
    const long long Cc = transpose ? Cin : Cout, Kc = transpose ? Cout : Cin;
    return 2ll * 9 * ((Kc + CK - 1) / CK) * CK * ((Cc + BM - 1) / BM) * BM;
}

extern "C" int idiff_pack_conv_weight_bf16(const float* w, void* out, int Cout, int Cin, int transpose, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(w && out && Cout > 0 && Cin > 0, "pack_conv_weight_bf16: bad args");
    IDIFF_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0, "pack_conv_weight_bf16: image must be 16-byte aligned");
    const long long n = idiff_conv_weight_bf16_bytes(Cout, Cin, transpose) / 2;
    const int ncob = ((transpose ? Cin : Cout) + BM - 1) / BM;
    const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, static_cast<__bf16*>(out), Cout, Cin, transpose, ncob, n);
    IDIFF_CHECK_LAUNCH("pack_conv_weight_bf16");
    return IDIFF_OK;
}
