/*
 * idiff.h -- C ABI of the MI355X-native InstanceDiff hot path (gfx950 HIP kernels).
 *
 * The reference (zyc-123/InstanceDiff) is pure Python: its "FFI" for this path is the YAML-keyed
 * plugin registry (models/__init__.py:4-12 -> create_net / create_sde) and every device kernel is an
 * implicit ATen/cuDNN dispatch.  Each entry point below names the reference call site(s) whose
 * implicit kernels it replaces.  The Python host side (instancediff_amd/) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers to fp32 unless stated; NCHW, contiguous inside a sample;
 *     "bstride" = elements between consecutive samples (lets a tensor be a channel slice of a bigger one)
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work (no sync, no alloc, no free)
 *   - caller owns every buffer, including workspaces; no pointer is retained after return
 *   - return 0 on success, <0 on error (IDIFF_E_*); idiff_last_error() gives a message
 */
#ifndef IDIFF_H
#define IDIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDIFF_OK 0
#define IDIFF_E_BADARG (-1)
#define IDIFF_E_UNSUPPORTED (-2)
#define IDIFF_E_HIP (-3)

typedef void* idiff_stream_t;

const char* idiff_last_error(void);
int idiff_version(void);
/* kernel launches this library has enqueued since it was loaded (bench.py reports launches per denoising step; under HIP-graph
 * capture the counter advances at capture time, not per replay) */
int64_t idiff_launch_count(void);
/* number of compute units etc. of the current device (plumbing for grid sizing / tests) */
int idiff_device_info(int* num_cu, int* wave_size, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the f32 matrix cores (v_mfma_f32_32x32x2_f32), NCHW fp32.
 * Replaces: every nn.Conv2d inside the (missing) UNet body -- ResBlock convs, init 7x7, final 3x3,
 * res 1x1, Down/Up-sample (call sites models/drift_noise_model.py:250-268).
 * ---------------------------------------------------------------------------------------------- */
#define IDIFF_CONV_NORMAL 0     /* out HxW = in HxW, pad = ks/2                                         */
#define IDIFF_CONV_UPSAMPLE2 1  /* nearest x2 upsample fused into the gather: out = 2Hin x 2Win         */
#define IDIFF_CONV_UNSHUFFLE2 2 /* pixel_unshuffle(2) fused: virtual Cin = 4*C0, out = Hin/2 x Win/2, ks=1 */

typedef struct {
    const float* src0;      /* [B, C0, Hin, Win]                                                      */
    const float* src1;      /* optional second source, channels appended after src0 (virtual concat)  */
    int64_t src0_bstride, src1_bstride;
    int32_t C0, C1;
    int32_t B, Hin, Win;
    int32_t mode;           /* IDIFF_CONV_*                                                            */
    int32_t ks;             /* 1, 3 or 7                                                               */
    int32_t Cout;
    const float* wpk;       /* packed weights [ks*ks][Cin][Cout] (idiff_pack_conv_weight)             */
    const float* bias;      /* [Cout] or NULL                                                          */
    /* prologue on src0 (requires C1 == 0): v = silu(pro_a[b,c]*v + pro_b[b,c]); zero padding applies
       AFTER the activation (it pads the activated tensor). NULL = raw input.                          */
    const float* pro_a;
    const float* pro_b;
    /* epilogue */
    float* out;             /* [B, Cout, Hout, Wout]                                                   */
    int64_t out_bstride;
    const float* res;       /* optional residual, same shape as out (res_bstride)                      */
    int64_t res_bstride;
    const float* vec;       /* optional per-(b,co) additive vector [B, Cout]                           */
    /* optional epilogue term: out += silu(aux_a[b,co]*aux[b,co,y,x] + aux_b[b,co])  (GN+SiLU of another tensor) */
    const float* aux;
    int64_t aux_bstride;
    const float* aux_a;
    const float* aux_b;
    float* stats;           /* optional GroupNorm partials [B][ntiles][Cout][2] (sum, sumsq) of the value
                               acc+bias, ntiles = idiff_conv2d_num_tiles(Hout,Wout)                     */
    const float* wwino;     /* optional Winograd-domain copy of the same 3x3 weights (idiff_pack_conv_weight_wino):
                               when set and the shape tiles exactly (Cin % 8 == 0 per source, Cout % 16 == 0,
                               Hout % 8 == 0, Wout % 32 == 0, NORMAL / UPSAMPLE2) the F(2x2,3x3) kernel runs
                               (2.25x fewer matrix-core flops, same epilogue); otherwise wpk is used       */
    const float* wwino4;    /* optional F(4x4,3x3)-domain copy (idiff_pack_conv_weight_wino4): preferred over wwino when
                               Hout % 4 == 0, Wout % 4 == 0, Wout >= 24, Cin % 8 == 0, Cout % 16 == 0 and a sample has at
                               least 16 items of 16x32 pixels x 64 channels (4x fewer matrix-core flops than direct) */
    /* Optional GroupNorm finalize of `stats` behind this conv (gn_out_a != NULL; requires stats): the per-(sample, channel) affine
       idiff_gn_finalize would compute, by an idiff_gn_finalize launch enqueued behind the conv by this call (one C call per conv +
       finalize).  Arguments as idiff_gn_finalize.  (r03 / r04 also had the finalize as the TAIL of the F(4x4,3x3) launches -- last
       arriving workgroups reducing the partials, bit-identical -- behind a `gn_ticket` field: measured slower in both rounds,
       +0.78 ms per step on the r04 kernel, and removed) */
    const float* gn_gamma;
    const float* gn_beta;
    const float* gn_film;
    int64_t gn_film_ld;
    float gn_eps;
    int32_t gn_groups;
    float* gn_out_a;
    float* gn_out_b;
    float* gn_mean_rstd;    /* optional [B, groups, 2] */
    int32_t algo_request;   /* 0 = the library picks (by the layer's per-sample shape only, never by the batch); 1 + IDIFF_CONV_ALGO_x =
                               run exactly that kernel or fail with IDIFF_E_ARG if the shape does not tile for it (a per-call
                               request: profiling, parity tests of a kernel at small sizes; a request for the F(4x4,3x3) kernel
                               waives its 16-items-per-sample threshold, nothing else); -(1 + IDIFF_CONV_ALGO_x) = prefer that
                               kernel where the shape tiles for it, the library's own choice elsewhere */
    const void* wx3;        /* ks == 1, normal mode: the weights split three ways into bf16 planes (idiff_pack_conv1x1_x3) or NULL.
                               With it, 1x1 layers whose pixels tile by 256 (Cout % 64 == 0, C0 % 8 == 0, Cin % 8 == 0, Cin >= 32, no prologue, no
                               statistics) run on the bf16 matrix cores with six products per fp32 product (IDIFF_CONV_ALGO_X3:
                               fp32-class result, csrc/conv1x1_x3.hip); NULL keeps them on the f32 matrix cores */
    /* ---- opt-in REDUCED-PRECISION 3x3 convs (IDIFF_CONV_ALGO_BF16, csrc/conv_bf16.hip, conv_bf16_wgrad.hip).  Both fields zero (the
       default) = the fp32 behaviour above, unchanged.  Numerics contract of the bf16 mode: every gathered input operand is computed in
       fp32 exactly as the f32 kernels compute it (virtual concat, nearest x2 upsample, prologue affine + SiLU, then zero padding); each
       operand and each weight is then rounded once to bf16 (round to nearest even, a plain cast); the products are summed in fp32 on
       the bf16 matrix cores; everything after the sum (bias, GroupNorm partials, vec, residual, aux term) is the fp32 epilogue.
       Eligible layers: ks == 3, NORMAL or UPSAMPLE2, Cout % 64 == 0, C0 % 32 == 0, C1 % 32 == 0, Hout % 8 == 0, Wout % 32 == 0;
       any other layer keeps the fp32 kernels (idiff_conv2d_last_algo says which ran). */
    const void* wbf16;      /* image of idiff_pack_conv_weight_bf16 (16-byte aligned; transpose = 1 for the data-gradient conv) */
    int32_t operands;       /* 0 = fp32 operands; 1 = bf16 operands on eligible 3x3 layers: the forward takes IDIFF_CONV_ALGO_BF16
                               when wbf16 is set too; idiff_conv2d_wgrad takes its bf16 form (the weight gradient needs no image) */
} idiff_conv_desc;

int idiff_conv2d_num_tiles(int Hout, int Wout);
int idiff_conv2d_fwd(const idiff_conv_desc* d, idiff_stream_t stream);
/* which kernel the calling thread's last idiff_conv2d_fwd launched (profiling / tests) */
#define IDIFF_CONV_ALGO_DIRECT 0   /* implicit GEMM, conv_igemm.hip  */
#define IDIFF_CONV_ALGO_WINOGRAD 1 /* F(2x2,3x3),   conv_wino.hip   */
#define IDIFF_CONV_ALGO_STREAM1X1 2 /* weight gradient only: streaming 1x1 product */
#define IDIFF_CONV_ALGO_WINOGRAD4 3 /* F(4x4,3x3),  conv_wino4.hip  */
#define IDIFF_CONV_ALGO_WINOGRAD4H 4 /* F(4x4,3x3), half-patch items, two workgroups per CU: conv_wino4h.hip */
#define IDIFF_CONV_ALGO_X3 5 /* 1x1, fp32 operands as three bf16 planes, six bf16 MFMAs per product: conv1x1_x3.hip */
#define IDIFF_CONV_ALGO_BF16 6 /* 3x3, operands rounded to bf16, fp32 sums (opt-in, idiff_conv_desc.operands): conv_bf16.hip */
int idiff_conv2d_last_algo(void);
/* Which kernel idiff_conv2d_fwd(d, .) WOULD launch for this descriptor: every check and selection rule of the call, no launch
 * (IDIFF_CONV_ALGO_* >= 0, or IDIFF_E_*).  The weight-image pointers of `d` only have to point at memory of the right size: a
 * caller whose weights change every step (training) asks first and then fills only the image the chosen kernel reads -- one pack
 * launch per use instead of three.  Does not change idiff_conv2d_last_algo(). */
int idiff_conv2d_plan(const idiff_conv_desc* d);
/* w [Cout][Cin] (the ks == 1 weight, torch layout) -> the three-plane bf16 image idiff_conv_desc.wx3 points to:
 * [chunk of 32 ci][block of 64 co][plane][octet of 8 ci][co][8 bf16], zero beyond Cin / Cout; x = plane0 + plane1 + plane2 exactly.
 * `image` holds idiff_conv1x1_x3_image_bytes(Cout, Cin) bytes, 16-byte aligned. */
long long idiff_conv1x1_x3_image_bytes(int Cout, int Cin);
int idiff_pack_conv1x1_x3(const float* w, void* image, int Cout, int Cin, idiff_stream_t stream);
/* w [Cout][Cin][ks][ks] (torch layout) -> wpk [ks*ks][Cin][Cout] */
int idiff_pack_conv_weight(const float* w, float* wpk, int Cout, int Cin, int ks, idiff_stream_t stream);
/* same, but spatially flipped and in/out swapped: wpk_T [ks*ks][Cout][Cin] for the data-gradient conv */
int idiff_pack_conv_weight_T(const float* w, float* wpk, int Cout, int Cin, int ks, idiff_stream_t stream);
/* 3x3 weights -> Winograd F(2x2,3x3) domain U = G g G^T, laid out as the kernel stages it:
 * [Cin/8][ceil(Cout/64)][16 xi][4 co-blocks][4 k][16 co][2]  (16*Cin*ceil(Cout/64)*64 floats; Cin % 8 == 0,
 * Cout % 16 == 0: a partial last block is zero-filled), Winograd rows
 * in the kernel's order (u0, u1, -u3, u2) -- an opaque image, only idiff_conv2d_fwd reads it.
 * transpose != 0: the flipped, in/out-swapped weights of the data-gradient conv (then the conv has Cin' = Cout, Cout' = Cin). */
int idiff_pack_conv_weight_wino(const float* w, float* wwino, int Cout, int Cin, int transpose, idiff_stream_t stream);
/* 3x3 weights -> Winograd F(4x4,3x3) domain (6x6 positions), laid out as conv_wino4.hip stages it:
 * [Cin/4][ceil(Cout/64)][9 position quads][4 co-blocks][4 k][16 co][4]  (36*Cin*ceil(Cout/64)*64 floats; Cin % 8 == 0,
 * Cout % 16 == 0: a partial last block is zero-filled) -- an opaque image, only idiff_conv2d_fwd reads it. */
int idiff_pack_conv_weight_wino4(const float* w, float* wwino4, int Cout, int Cin, int transpose, idiff_stream_t stream);
/* 3x3 weights w [Cout][Cin][3][3] (torch layout) -> the bf16 image idiff_conv_desc.wbf16 points to, each weight rounded once to
 * bf16 (nearest even): [chunk of 32 ci][block of 64 co][tap][octet of 8 ci][co][8 bf16] of the conv's (Cout, Cin), zero beyond them.
 * transpose != 0: the flipped, in/out-swapped weights of the data-gradient conv (the conv's Cout' = Cin, Cin' = Cout).  `image` holds
 * idiff_conv_weight_bf16_bytes(Cout, Cin, transpose) bytes, 16-byte aligned. */
long long idiff_conv_weight_bf16_bytes(int Cout, int Cin, int transpose);
int idiff_pack_conv_weight_bf16(const float* w, void* image, int Cout, int Cin, int transpose, idiff_stream_t stream);
/* Layers with fewer than 16 items PER SAMPLE (16x32 pixels x 64 output channels each) stay on the F(2x2,3x3) kernel; the batch
 * size never enters the choice (a sample's bits do not depend on its batch).  There is no process-wide switch: a caller that
 * wants another kernel for ONE call says so in idiff_conv_desc.algo_request. */

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+FiLM) folded to a per-(sample,channel) affine, applied by the consumer kernel.
 * Replaces: nn.GroupNorm + x*(scale+1)+shift inside every ResBlock.
 *   mean/var per (b,group) from the conv partials (fp64 finalize), then
 *   a[b,c] = rstd*gamma[c]*(1+scale[b,c]);  b[b,c] = (beta[c]-mean*rstd*gamma[c])*(1+scale[b,c]) + shift[b,c]
 *   film: [B, 2C] (scale = film[b, c], shift = film[b, C+c], row stride film_ld) or NULL.
 *   mean_rstd (optional out): [B, groups, 2] for the backward pass.
 * ---------------------------------------------------------------------------------------------- */
int idiff_gn_finalize(const float* stats, int ntiles, int B, int C, int groups, int HW, const float* gamma,
                      const float* beta, const float* film, int64_t film_ld, float eps, float* out_a, float* out_b,
                      float* mean_rstd, idiff_stream_t stream);

/* out[b,c,p] = silu(a[b,c]*h[b,c,p] + b[b,c]) + res[b,c,p] + vec[b,c]   (res, vec, a/b optional)
 * Replaces: GroupNorm->SiLU->(+residual) tail of each ResBlock and the M=1 cross-attention add. */
int idiff_affine_silu_add(const float* h, int64_t h_bstride, const float* a, const float* b, const float* res,
                          int64_t res_bstride, const float* vec, float* out, int64_t out_bstride, int B, int C, int HW,
                          idiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Token-side ops (small row counts): Linear, LayerNorm, sinusoidal time embedding.
 * Replaces: timestep-embedding MLP, per-ResBlock time projections, image-context K/V projections and
 * the ScoreMapModule text branch (_modified_BiomedCLIP.py:531-541,1205-1223).
 * ---------------------------------------------------------------------------------------------- */
#define IDIFF_ACT_NONE 0
#define IDIFF_ACT_SILU 1
#define IDIFF_ACT_GELU 2
/* out[r, n] = res[r,n] + gscale[n] * ( sum_k act_in(x[r,k]) * w[n,k] + bias[n] ), then act_out.
 * x: [R, K] row stride ldx; w: [N, K] row stride ldw (torch nn.Linear layout); out row stride ldo;
 * res (row stride ldr), bias, gscale optional (NULL). */
int idiff_linear_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res,
                     int64_t ldr, const float* gscale, float* out, int64_t ldo, int R, int K, int N, int act_in,
                     int act_out, idiff_stream_t stream);
/* same contract with a PRE-TRANSPOSED weight wT [K, N] (row stride ldw): lane = output feature, unit-stride weight
 * reads, no cross-lane reduction -- the low-latency form used for the ScoreMapModule token chain.
 * The rows of x are staged in LDS: K <= 2044 on the matrix-core kernel (N % 4 == 0, ldw % 4 == 0, wT 16-byte aligned), K <= 4864 on the
 * vector kernel that takes every other shape (160 KiB of LDS per workgroup); a larger K returns IDIFF_E_UNSUPPORTED (IDIFF_E_BADARG
 * beyond 8192). */
int idiff_linear_t_fwd(const float* x, int64_t ldx, const float* wT, int64_t ldw, const float* bias, const float* res,
                       int64_t ldr, const float* gscale, float* out, int64_t ldo, int R, int K, int N, int act_in,
                       int act_out, idiff_stream_t stream);
/* Up to IDIFF_LINEAR_MAX_GROUPS independent idiff_linear_t_fwd / idiff_linear_t_ln_fwd problems (own operands and shapes; ln_g == NULL:
 * no LayerNorm) in ONE launch: the same token-side linear of the ScoreMapModules of all four UNet levels, or of the heads of one
 * folded projection.  Latency-bound launches of ~10 us each: one grouped launch costs what one of them did.  The descriptors are
 * copied into the kernel arguments (nothing is retained).  Matrix-core form only: N % 4 == 0, ldw % 4 == 0, wT 16-byte aligned. */
#define IDIFF_LINEAR_MAX_GROUPS 16
typedef struct {
    const float* x;       /* [R, K], row stride ldx */
    int64_t ldx;
    const float* wT;      /* [K, N] pre-transposed weight, row stride ldw */
    int64_t ldw;
    const float* bias;    /* [N] or NULL */
    const float* res;     /* [R, N] residual (row stride ldr) or NULL */
    int64_t ldr;
    const float* gscale;  /* [N] per-column gain or NULL */
    float* out;           /* [R, N], row stride ldo */
    int64_t ldo;
    const float* ln_g;    /* LayerNorm over K in front of the product (with ln_b; act_in must be IDIFF_ACT_NONE) or NULL */
    const float* ln_b;
    float ln_eps;
    int32_t R, K, N, act_in, act_out;
} idiff_linear_group;
int idiff_linear_t_grouped_fwd(const idiff_linear_group* groups, int ngroups, idiff_stream_t stream);
/* idiff_linear_t_fwd on LayerNorm(x) (per row over K, parameters ln_g / ln_b [K]): the LayerNorm runs on the rows the
 * kernel has staged anyway -- the LayerNorm -> Linear pairs of the ScoreMapModule decoder in one launch each. */
int idiff_linear_t_ln_fwd(const float* x, int64_t ldx, const float* ln_g, const float* ln_b, float ln_eps, const float* wT,
                          int64_t ldw, const float* bias, const float* res, int64_t ldr, const float* gscale, float* out,
                          int64_t ldo, int R, int K, int N, int act_out, idiff_stream_t stream);
/* `heads` independent products of that form in ONE launch (no res / gscale / activation): head h uses x + h*x_hs,
 * wT + h*w_hs, bias + h*b_hs, out + h*o_hs -- the per-head k/v folds of the ScoreMapModule cross-attention, whose
 * operands are column / row blocks of shared matrices. */
int idiff_linear_t_heads_fwd(const float* x, int64_t ldx, int64_t x_hs, const float* wT, int64_t ldw, int64_t w_hs,
                             const float* bias, int64_t b_hs, float* out, int64_t ldo, int64_t o_hs, int R, int K, int N,
                             int heads, idiff_stream_t stream);
/* ScoreMapModule memory projection fused in one pass (ContextDecoder.memory_proj, _modified_BiomedCLIP.py:1205-1209):
 * out[b,:,p] = LayerNorm_256( wpk^T . LayerNorm_C(feat[b,:,p]) + bias );  feat [B,C,N] (feat_bstride), wpk [C][256]
 * (idiff_pack_conv_weight of the [256,C,1,1] view), out [B,256,N]. */
int idiff_smm_memproj_fwd(const float* feat, int64_t feat_bstride, const float* ln1_g, const float* ln1_b,
                          const float* wpk, const float* bias, const float* ln2_g, const float* ln2_b, float* out, int B,
                          int C, int N, float eps, idiff_stream_t stream);
/* Compact form of the same memory for narrow feature maps (C + 1 <= Cm < 256).  With xhat = LayerNorm_C(feat[b,:,p]),
 * z = W.xhat + bias, rstd = 1/sqrt(var(z)+eps2):   LayerNorm_256(z) = g2 * ((Wc.xhat + bc) * rstd) + b2
 * (Wc, bc = W and bias centred over the 256 outputs), i.e. the 256-wide memory is an affine image of the (C+1)-vector
 * [xhat*rstd ; rstd].  out [B,Cm,N] = rows [xhat*rstd (C) ; rstd (1) ; zeros]; the host folds g2.[Wc|bc] into the query
 * and value projections of the cross-attention (b2 cancels in the softmax and re-enters as a bias), so
 * idiff_smm_xattn_fwd streams (C+1)/256 of the bytes.  The variance itself is evaluated as the quadratic form
 * var = xhat^T G xhat + 2 h.xhat + e with  gram = Wc^T Wc / 256  [C][C],  hvec = Wc^T bc / 256  [C],  evar = |bc|^2 / 256
 * (host-prepared in fp64): a C -> C product instead of C -> 256.  Same arithmetic as idiff_smm_memproj_fwd up to fp32
 * rounding.  C = 64 or 128 (a thread holds C / 4 channels of its pixel in registers). */
int idiff_smm_memproj_compact_fwd(const float* feat, int64_t feat_bstride, const float* ln1_g, const float* ln1_b,
                                  const float* gram, const float* hvec, float evar, float* out, int B, int C, int N, int Cm,
                                  float eps1, float eps2, idiff_stream_t stream);
/* Training step (r05): the same projection with the quadratic form's constant read from device memory (it is a function of the
 * weights, evaluated on the device every step), C = 64, and its backward.  Given dm [B, Cm, N] (rows 0..C carry gradient):
 *   dfeat [B, C, N] (dfeat_bstride) and dparams [C*C + 3C + 1] = d gram (row-major) | d ln1_g | d ln1_b | d hvec | d evar.
 * ws: idiff_smm_memproj_compact_bwd_ws_floats(B, C, N) floats (per-workgroup partial rows, reduced in a fixed order).
 * Limits: both training entry points take C = 64 only (C = 128, which idiff_smm_memproj_compact_fwd accepts, is IDIFF_E_BADARG) and
 * Cm > C; the forward also needs N % 4 == 0 and feat_bstride % 4 == 0.  The backward reads rows 0..C of dm and ignores the rest. */
int idiff_smm_memproj_compact_train_fwd(const float* feat, int64_t feat_bstride, const float* ln1_g, const float* ln1_b, const float* gram,
                                        const float* hvec, const float* evar_dev, float* out, int B, int C, int N, int Cm, float eps1,
                                        float eps2, idiff_stream_t stream);
int64_t idiff_smm_memproj_compact_bwd_ws_floats(int B, int C, int N);
int idiff_smm_memproj_compact_bwd(const float* feat, int64_t feat_bstride, const float* ln1_g, const float* ln1_b, const float* gram,
                                  const float* hvec, const float* evar_dev, const float* dm, float* dfeat, int64_t dfeat_bstride,
                                  float* dparams, float* ws, int B, int C, int N, int Cm, float eps1, float eps2, idiff_stream_t stream);
/* Several idiff_smm_memproj_compact_fwd problems (the ScoreMapModules of a net's levels) in ONE launch; same arithmetic per problem,
 * same bits.  The launch reserves the LDS of its widest problem: group levels of equal C. */
#define IDIFF_MEMPROJ_MAX_GROUPS 4
typedef struct idiff_memproj_group {
    const float* feat;
    int64_t feat_bstride;
    const float *ln1_g, *ln1_b, *gram, *hvec;
    float evar;
    float* out;
    int32_t C, N, Cm;
} idiff_memproj_group;
int idiff_smm_memproj_compact_grouped_fwd(const idiff_memproj_group* groups, int ngroups, int B, float eps1, float eps2,
                                          idiff_stream_t stream);
int idiff_layernorm_rows_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out,
                             int64_t ldo, int R, int C, float eps, float* mean_rstd, idiff_stream_t stream);
/* sinusoidal embedding, [sin | cos] halves; freqs [dim/2] = host-built table exp(-ln(1e4) * i/(half-1))
 * (NULL = computed on device) */
int idiff_time_embed_fwd(const float* t, const float* freqs, int B, int dim, float* out, idiff_stream_t stream);
/* The UNet's time-embedding MLP (frozen spec, DESIGN.md section 2: temb = Linear(GELU(Linear(sinusoidal_dim(t))))) in ONE launch:
 * out [B, nout] = w2 . GELU(w0 . [sin(t f) ; cos(t f)] + b0) + b2 with w0 [hid, dim], w2 [nout, hid] (torch layout), freqs [dim/2] or
 * NULL; dim = 64, hid = 256, nout <= 256 (the UNet's nf = 64).  The sums run in a different order than the
 * idiff_time_embed_fwd -> idiff_linear_fwd(act_out = GELU) -> idiff_linear_fwd chain it replaces (fp32 rounding differences only). */
int idiff_time_mlp_fwd(const float* t, const float* freqs, const float* w0, const float* b0, const float* w2, const float* b2, float* out,
                       int B, int dim, int hid, int nout, idiff_stream_t stream);

/* LayerNorm over the channel dim of an NCHW map (per pixel). Replaces the pre-norm of attention blocks. */
int idiff_chan_layernorm_fwd(const float* x, int64_t x_bstride, const float* gamma, const float* beta, float* out,
                             int64_t out_bstride, int B, int C, int HW, float eps, float* mean_rstd,
                             idiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention.  All follow _modified_BiomedCLIP.py:464-478:  softmax(q k^T * scale) v  per head.
 * ---------------------------------------------------------------------------------------------- */
/* self-attention over a feature map: qkv [B, 3C, N] channel-major (q rows 0..C-1, k C..2C-1, v 2C..3C-1),
 * out [B, C, N]; head h owns channels h*dh..(h+1)*dh-1; dh must be 64 or 32 and N a multiple of 4 (16-byte key loads);
 * flash-style on f32 MFMA.
 * lse (optional) [B, heads, N] = log-sum-exp per query for the backward pass. */
int idiff_attn_self_fwd(const float* qkv, float* out, float* lse, int B, int C, int N, int heads, float scale,
                        idiff_stream_t stream);
/* REDUCED-PRECISION VARIANT of idiff_attn_self_fwd (off by default; BASELINE config c5 "fp16 MFMA attention"): Q K^T and P V on
 * the bf16 matrix cores, fp32 softmax and accumulation; head dim 64.  Reported by bench.py as a separate, labelled line. */
int idiff_attn_self_bf16_fwd(const float* qkv, float* out, int B, int C, int N, int heads, float scale, idiff_stream_t stream);
/* the same with fp16 operands clamped to +-255 before the cast -- the reference's own half-precision form (flash-attn branch,
 * models/_modified_BiomedCLIP.py:509-513; BASELINE config c5 "fp16 MFMA attention"); labelled variant, off by default */
int idiff_attn_self_f16_fwd(const float* qkv, float* out, int B, int C, int N, int heads, float scale, idiff_stream_t stream);
/* pixels attend to M context tokens: q [B,C,N] channel-major, k,v [B,M,C] token-major, out [B,C,N]; M <= 32 */
int idiff_attn_ctx_fwd(const float* q, const float* k, const float* v, float* out, int B, int C, int N, int M,
                       int heads, float scale, idiff_stream_t stream);
/* tiny token-major attention (ScoreMapModule decoder self-attention): q [B,Nq,C] (row stride ldq), k,v [B,M,C]
 * (row stride ldkv) -- strides let q/k/v be slices of one packed qkv projection; out [B,Nq,C] dense; M <= 64 (a lane per key);
 * Nq is not limited (a wave per query); any head dim C / heads */
int idiff_attn_tokens_fwd(const float* q, const float* k, const float* v, float* out, int B, int Nq, int M, int C,
                          int heads, float scale, int64_t ldq, int64_t ldkv, idiff_stream_t stream);
/* Backward of idiff_attn_tokens_fwd for few tokens -- the class-token self-attention of the ScoreMapModule decoder in the training
 * step: P is recomputed, dq/dk/dv [rows, C] with row strides lddq / lddkv (packed q|k|v buffers allowed).
 * Limits (narrower than the forward's; anything else is IDIFF_E_BADARG before any launch): 1 <= Nq <= 8 and 1 <= M <= 8 (the kernel
 * unrolls both loops to 8), head dim C / heads <= 64 (a lane per channel of the head), C % heads == 0, every row stride
 * (ldq, ldkv, ldo, lddq, lddkv) >= C, no null pointer.  k and v share ldkv, dk and dv share lddkv. */
int idiff_attn_tokens_bwd(const float* q, const float* k, const float* v, const float* d_o, float* dq, float* dk, float* dv, int B, int Nq,
                          int M, int C, int heads, float scale, int64_t ldq, int64_t ldkv, int64_t ldo, int64_t lddq, int64_t lddkv,
                          idiff_stream_t stream);
/* idiff_attn_tokens_fwd for ngroups (<= IDIFF_LINEAR_MAX_GROUPS) operand sets of one shape in ONE launch (host arrays of device pointers) */
int idiff_attn_tokens_grouped_fwd(const float* const* q, const float* const* k, const float* const* v, float* const* out, int ngroups,
                                  int B, int Nq, int M, int C, int heads, float scale, int64_t ldq, int64_t ldkv, idiff_stream_t stream);
/* The reference's half-precision attention form for the ScoreMapModule decoder (Attention_flash, models/_modified_BiomedCLIP.py:481-517,
 * selected by TransformerDecoderLayer_scaled(if_flash=True), :552-590): q / k / v clamped to +-255 and rounded to fp16, fp32 scores and
 * softmax statistics, probabilities rounded to fp16 for the second product, fp32 accumulation, result rounded to fp16 (returned as
 * fp32).  Labelled REDUCED-PRECISION VARIANT (model option score_map_if_flash, inference only); csrc/attention_flash.hip.
 * idiff_attn_tokens_f16_fwd: the operands of idiff_attn_tokens_fwd.
 * idiff_smm_xattn_kv_f16_fwd: q [B, Nq, heads*64] (after q_proj), k, v [B, heads*64, N] channel-major (after k_proj / v_proj: unfolded --
 * the folded form has no k / v tensor to clamp), out [B, Nq, heads*64]; heads == 4, Nq <= 8, N % 4 == 0;
 * ws: idiff_smm_xattn_kv_f16_ws_floats(B, N) floats. */
int idiff_attn_tokens_f16_fwd(const float* q, const float* k, const float* v, float* out, int B, int Nq, int M, int C, int heads, float scale,
                              int64_t ldq, int64_t ldkv, idiff_stream_t stream);
int64_t idiff_smm_xattn_kv_f16_ws_floats(int B, int N);
int idiff_smm_xattn_kv_f16_fwd(const float* q, const float* k, const float* v, float* out, float* ws, int B, int Nq, int heads, int C, int N,
                               float scale, idiff_stream_t stream);
/* ScoreMapModule cross-attention, K/V projections folded onto the query side:
 *   S[b,h,q,n] = scale * sum_c qf[b,q,h,c] * mem[b,c,n];  P = softmax_n(S);  o[b,q,h,c] = sum_n P * mem[b,c,n]
 * qf, o: [B, Nq, heads, Cm];  mem: [B, Cm, N] channel-major;  Nq*heads <= 32, Cm in {72, 136, 256}.
 * ws: workspace of idiff_smm_xattn_ws_floats(B,Nq,heads,Cm,N) floats. */
int64_t idiff_smm_xattn_ws_floats(int B, int Nq, int heads, int Cm, int N);
int idiff_smm_xattn_fwd(const float* qf, const float* mem, float* o, float* ws, int B, int Nq, int heads, int Cm,
                        int N, float scale, idiff_stream_t stream);
/* Up to IDIFF_XATTN_MAX_GROUPS independent idiff_smm_xattn_fwd problems of one (B, Nq, heads, scale) -- the cross-attentions of a
 * net's four ScoreMapModules in one decoder layer -- in ONE attention launch and ONE merge launch.  Each problem keeps the kernel,
 * the key split and the merge order of its single launch: the results are the same bits.  ws per problem as for the single call. */
#define IDIFF_XATTN_MAX_GROUPS 8
typedef struct idiff_xattn_group {
    const float* qf;   /* [B, Nq, heads, Cm] */
    const float* mem;  /* [B, Cm, N] */
    float* o;          /* [B, Nq, heads, Cm] */
    float* ws;         /* idiff_smm_xattn_ws_floats(B, Nq, heads, Cm, N) floats */
    int32_t Cm, N;
} idiff_xattn_group;
int idiff_smm_xattn_grouped_fwd(const idiff_xattn_group* groups, int ngroups, int B, int Nq, int heads, float scale,
                                idiff_stream_t stream);
/* Training path of the same attention over the full 256-row memory (Cm = 256, rows = Nq*heads <= 32, row-major qf / o [B, rows, 256]):
 * the forward also returns lse [B, rows] (log-sum-exp of the scaled scores); the backward makes ONE pass over the keys,
 *   dP = do mem, D = rowsum(do*o), G = scale * P * (dP - D), dqf = G mem^T, dmem = do^T P + qf^T G     (P = exp(scale*qf mem - lse)),
 * replacing the batched-GEMM / softmax chains autograd derived (each of which streamed the [B,256,N] memory or [B,rows,N] scores).
 * ws: idiff_smm_xattn_ws_floats(B, rows, 1, 256, N) floats for either call; dmem [B,256,N] is overwritten, or added to when
 * accumulate != 0 (the decoder layers of a ScoreMapModule attend to one memory: their gradients are summed in place, in call order). */
int idiff_smm_xattn_lse_fwd(const float* qf, const float* mem, float* o, float* lse, float* ws, int B, int rows, int N, float scale,
                            idiff_stream_t stream);
int idiff_smm_xattn_bwd(const float* qf, const float* mem, const float* o, const float* lse, const float* d_o, float* dqf, float* dmem,
                        int accumulate, float* ws, int B, int rows, int N, float scale, idiff_stream_t stream);
/* The same pair over a memory of Cm rows (row-major qf / o / dqf [B, rows, Cm], mem / dmem [B, Cm, N]): Cm = 256, or 72 for the compact
 * (C + 1)-row memory of the 64-channel levels (r05: the training step attends to the compact memory too; its padding rows carry no
 * gradient).  ws: idiff_smm_xattn_ws_floats(B, rows, 1, Cm, N) floats.
 * Limits of both backward entry points: 1 <= rows <= 32, N % 4 == 0, and Cm = 72 or 256 only -- Cm = 136, which the forward
 * (idiff_smm_xattn_fwd / _cm_lse_fwd) accepts, is refused with IDIFF_E_BADARG (the 128-channel levels train on the 256-row memory). */
int idiff_smm_xattn_cm_lse_fwd(const float* qf, const float* mem, float* o, float* lse, float* ws, int B, int rows, int Cm, int N,
                               float scale, idiff_stream_t stream);
int idiff_smm_xattn_cm_bwd(const float* qf, const float* mem, const float* o, const float* lse, const float* d_o, float* dqf, float* dmem,
                           int accumulate, float* ws, int B, int rows, int Cm, int N, float scale, idiff_stream_t stream);
/* score map: out[b,k,p] = <feat[b,:,p]/max(|feat[b,:,p]|,eps), tv[b,k,:]/max(|tv[b,k,:]|,eps)>; K <= 8
 * sel (optional) [B, HW] = out[b, idx[b], :]  (idx int32 [B]) */
int idiff_scoremap_fwd(const float* feat, int64_t feat_bstride, const float* tv, float* out, const int32_t* idx,
                       float* sel, int B, int C, int HW, int K, idiff_stream_t stream);
/* The score maps of several levels in ONE launch (same K, idx); 16-byte form only (HW % 4 == 0, aligned operands). */
#define IDIFF_SCOREMAP_MAX_GROUPS 4
typedef struct idiff_scoremap_group {
    const float* feat;
    int64_t feat_bstride;
    const float* tv;  /* [B, K, C] */
    float* out;       /* [B, K, HW] */
    float* sel;       /* [B, HW] or NULL (with idx) */
    int32_t C, HW;
} idiff_scoremap_group;
int idiff_scoremap_grouped_fwd(const idiff_scoremap_group* groups, int ngroups, const int32_t* idx, int B, int K, idiff_stream_t stream);
/* Output layer fused with the class gather (replaces the UNet's final 3x3 conv to out_nc channels followed by the
 * per-sample channel pick): out[b,0,y,x] = bias[idx[b]] + sum_{ci,ky,kx} w[idx[b],ci,ky,kx] * x[b,ci,y+ky-1,x+kx-1]
 * w [K,C,3,3] (torch layout), bias [K] or NULL, idx int32 [B] in [0,K), out [B,1,H,W]. */
int idiff_conv3x3_select_fwd(const float* x, int64_t x_bstride, const float* w, const float* bias, const int32_t* idx, float* out,
                             int B, int C, int K, int H, int W, idiff_stream_t stream);
/* Its backward (training step): dx [B,C,H,W] (dx_bstride) = the transposed conv of dpred [B,1,H,W] with each sample's class kernel,
 * dw [K,C,3,3] / db [K] (db may be NULL) = sums over the samples of each class (classes without a sample get zeros); either of dx / dw
 * may be NULL.  W % 4 == 0.  ws: idiff_conv3x3_select_bwd_ws_floats(B, C, H, W) floats (per-tile partials, reduced in a fixed order).
 * Every argument is checked before the first launch: a call that returns IDIFF_E_BADARG (a missing ws with dw set included) has
 * written nothing, dx included. */
int64_t idiff_conv3x3_select_bwd_ws_floats(int B, int C, int H, int W);
int idiff_conv3x3_select_bwd(const float* x, int64_t x_bstride, const float* w, const int32_t* idx, const float* dpred, float* dx,
                             int64_t dx_bstride, float* dw, float* db, float* ws, int B, int C, int K, int H, int W, idiff_stream_t stream);
/* out[b,0,p] = x[b, idx[b], p] */
int idiff_gather_channel(const float* x, const int32_t* idx, float* out, int B, int C, int HW, idiff_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SDE updates.  Replaces the 4-6 ATen elementwise launches + randn_like per step of
 * utils/sde_utils.py:45-46,178-188,196-199 (IRSDE) and the driftSDE reverse update.
 * Noise: z != NULL -> injected draws (parity mode); z == NULL -> on-device Philox4x32-10 + Box-Muller
 * keyed by (seed, offset) (throughput mode).
 * ---------------------------------------------------------------------------------------------- */
#define IDIFF_SDE_STEP 0  /* reverse_sde_step       (sde_utils.py:45-46)  */
#define IDIFF_SDE_MEAN 1  /* reverse_sde_step_mean  (:41-42)              */
#define IDIFF_SDE_ODE 2   /* reverse_ode_step       (:48-49,181-182)      */
/* x_out = x - (theta*(mu-x) - coef*sigma^2*score)*dt [- sigma*(z*sqrt_dt)],  score = -noise_pred/sigma_bar;
 * same fp32 operation order as the reference (bit-exact given identical z). */
int idiff_irsde_reverse_step(const float* x, const float* mu, const float* noise_pred, const float* z, float* x_out,
                             int64_t n, float theta, float sigma, float sigma_bar, float dt, float sqrt_dt, int mode,
                             uint64_t seed, uint64_t offset, idiff_stream_t stream);
/* The pieces the reference composes its steps and closed forms from, one launch each, every product / sum / quotient rounded
 * once in the reference's order (bit-exact against the CPU reference given identical draws).  Operands a, b, z are [B][per]
 * (NULL where an op does not read them; z == NULL on an op that draws noise -> Philox keyed by (seed, offset));
 * mu NULL -> the scalar mu_scalar (the reference's default `self.mu = 0.`, sde_utils.py:152).
 * Coefficients k[0..5]: by value in `k` when coef_dev == NULL (python-int t), else per-sample device rows coef_dev[B][6]
 * (t given as a [B,1,1,1] tensor, sde_utils.py:330-336).  The host fills them from the schedule tables. */
#define IDIFF_IRSDE_SCORE_FROM_NOISE 0 /* get_score_from_noise :187-188   (-a) / k0                       k0 = sigma_bar_t        */
#define IDIFF_IRSDE_MU_BAR 1           /* mu_bar :169-170                  mu + (a - mu)*k0                k0 = exp(-cumsum_t dt)  */
#define IDIFF_IRSDE_DRIFT 2            /* drift :175-176                   (k0*(mu - a))*k1                k0 = theta_t, k1 = dt   */
#define IDIFF_IRSDE_REV_DRIFT 3        /* sde_/ode_reverse_drift :178-182  (k0*(mu - a) - k1*b)*k2         k1 = sigma_t^2 [*0.5], k2 = dt */
#define IDIFF_IRSDE_DISPERSION 4       /* dispersion :184-185              k0*(z*k1)                       k0 = sigma_t, k1 = sqrt(dt) */
#define IDIFF_IRSDE_STEP_MEAN 5        /* reverse_sde_step_mean / reverse_ode_step :41-42,48-49   a - REV_DRIFT(a, b)              */
#define IDIFF_IRSDE_STEP_SDE 6         /* reverse_sde_step :45-46          (a - REV_DRIFT(a, b)) - k3*(z*k4)   k3 = sigma_t, k4 = sqrt(dt) */
#define IDIFF_IRSDE_FORWARD_STEP 7     /* forward_step :38-39              (a + (k0*(mu - a))*k1) + k3*(z*k4)                      */
#define IDIFF_IRSDE_OPT_STEP 8         /* reverse_optimum_step :206-214    ((k0*(a - mu)) + (k1*(b - mu))) + mu   k0 = term1, k1 = term2 */
#define IDIFF_IRSDE_REAL_NOISE 9       /* get_real_noise :222-223          (a - (mu + (b - mu)*k0)) / k1   k1 = sigma_bar_t        */
#define IDIFF_IRSDE_REAL_SCORE 10      /* get_real_score :225-226          (-(a - (mu + (b - mu)*k0))) / k1   k1 = sigma_bar_t^2   */
#define IDIFF_IRSDE_INIT_FROM_NOISE 11 /* get_init_state_from_noise :228-230   (((a - mu) - k0*b)*k1) + mu   k0 = sigma_bar_t, k1 = exp(+cumsum_t dt) */
#define IDIFF_IRSDE_RANDOM_STATES 12   /* generate_random_states :333-336  (z*k1) + (mu + (a - mu)*k0)     k0 = exp(-cumsum_t dt), k1 = sigma_bar_t */
#define IDIFF_IRSDE_NUM_OPS 13
int idiff_irsde_map(int op, const float* a, const float* b, const float* z, const float* mu, float mu_scalar, float* out, int B,
                    int64_t per_sample, const float* coef_dev, const float* k, uint64_t seed, uint64_t offset,
                    idiff_stream_t stream);
/* x_out = ((x - a*r_hat) - b*e_hat) + c*z ;  xa_out (optional) = x_out - cond  (next step's network input) */
int idiff_drift_reverse_step(const float* x, const float* r_hat, const float* e_hat, const float* z, const float* cond,
                             float* x_out, float* xa_out, int64_t n, float a, float b, float c, uint64_t seed,
                             uint64_t offset, idiff_stream_t stream);
/* Graph-replayable drift step: all per-step scalars live in device memory, so ONE captured HIP graph of a denoising step
 * (two UNet forwards + this update + idiff_step_state_advance) replays for every t with no host input in between.
 *   state int32[3] = {t, Philox call count, step index of this run};  coef float[3][Tp1] = tables of (a_t, b_t, c_t);
 *   a, b, c = coef[.][t];  Philox offset = offset_base + state[1]*nper (offset_base: the counters this stream's earlier draws, of
 *   whatever size, have consumed -- successive draws never share counters);  z_base (optional, parity runs) [steps][n] indexed by state[2].
 * In place:  x <- ((x - a*r_hat) - b*e_hat) + c*z ;  xa <- x - cond.   Same fp32 operation order as idiff_drift_reverse_step. */
int idiff_drift_reverse_step_dev(float* x, const float* r_hat, const float* e_hat, const float* z_base, const float* cond,
                                 float* xa, int64_t n, const float* coef, int Tp1, const int32_t* state, uint64_t seed,
                                 uint64_t nper, uint64_t offset_base, idiff_stream_t stream);
/* Second-order multistep form of idiff_drift_reverse_step_dev (driftSDE solver_order = 2): each prediction is
 * extrapolated linearly from the previous jump's before the same update, at no extra network evaluation.
 *   coef5 float[5][Tp1] = tables of (a, b, c, rho_d, rho_s), read at t = state[0];  state, seed, nper, offset_base and z_base are those
 *   of idiff_drift_reverse_step_dev: for the same (seed, offset_base, state) the two entry points draw the same z.
 *   r_prev, e_prev [n]: the previous jump's r_hat / e_hat, kept by this call at fixed addresses for the next replay.  They must be
 *   distinct from each other and from every other operand.
 * fp32 operation order, one rounding per operation, no contraction:
 *   R~ = r_hat + rho_d*(r_hat - r_prev)        (R~ = r_hat and r_prev is not read when rho_d == 0)
 *   e~ = e_hat + rho_s*(e_hat - e_prev)        (e~ = e_hat and e_prev is not read when rho_s == 0)
 *   x  <- ((x - a*R~) - b*e~) + c*z ;   xa <- x - cond ;   r_prev <- r_hat ;   e_prev <- e_hat        (all in place)
 * With rho_d == rho_s == 0 (the first jump of a chain) the result is bit-identical to idiff_drift_reverse_step_dev with the same a, b, c
 * whatever the history holds, uninitialised memory and NaNs included.  A NaN rho (a row that starts no jump) counts as non-zero. */
int idiff_drift_reverse_step2_dev(float* x, const float* r_hat, const float* e_hat, float* r_prev, float* e_prev, const float* z_base,
                                  const float* cond, float* xa, int64_t n, const float* coef5, int Tp1, const int32_t* state,
                                  uint64_t seed, uint64_t nper, uint64_t offset_base, idiff_stream_t stream);
/* ---- posterior ensembles: member noise streams ----
 * Philox4x32-10 takes a 128-bit counter; every entry point above uses 64 bits of it (words c2 = c3 = 0).  A member stream uses the rest:
 *   counter words (c0, c1, c2, c3) = (lo32(q), hi32(q), lo32(m), hi32(m)),  key = seed,  word -> normal mapping as in idiff_randn;
 *   m = member id >= 1 (m = 0 is the stream of the entry points above; the host wrappers refuse it, so no member stream overlaps it);
 *   q = j*Q + v,  Q = n_s/4,  n_s = elements of ONE sample (n_s % 4 != 0 is an error),  v = 4-element group inside the sample,
 *   j = 0: the member's x_T draw;  j = 1 + state[1]: the z of a step.
 * A member's noise is a function of (seed, m, j) alone: not of its row, of the rows beside it, or of earlier draws.
 * members_dev: uint64 ids on the device, one per row.  Rows are n_s contiguous floats, all operands 16-byte aligned, rows <= 65535. */
/* out[r, :] = normals of member members_dev[r] at draw index j */
int idiff_randn_members(float* out, int R, int64_t n_s, const uint64_t* members_dev, uint64_t seed, uint64_t j, idiff_stream_t stream);
/* row b*S + s:  cond_rep = cond[b] ;  x = 1*cond + sigma*z(member, j = 0) ;  xa = x - cond.   Bit-identical to idiff_randn_members followed
 * by idiff_axpby(cond_rep, z, 1, sigma) and idiff_axpby(x, cond_rep, 1, -1). */
int idiff_ensemble_init(const float* cond, float* cond_rep, float* x, float* xa, int B, int S, int64_t n_s, const uint64_t* members_dev,
                        float sigma, uint64_t seed, idiff_stream_t stream);
/* The start of an image in a chain whose buffers and captured step graph outlive the call (driftSDE reuse_graph): the
 * x_T construction into the chain's own cond / x / xa and the device state of its first step, in ONE launch.
 * Plain chain (members_dev == NULL): S == 1, row0 == 0, R == B are required; n = B*n_s >= 1 is any size (a tail of n % 4 elements is
 *   handled element-wise, as in idiff_randn).  z is the library's one stream at counters offset + v over the flattened batch:
 *   cond = cond_in ;  x = 1*cond_in + sigma*z ;  xa = x - cond_in, bit-identical to idiff_randn(z, n, seed, offset) followed by
 *   idiff_axpby(cond_in, z, 1, sigma) and idiff_axpby(x, cond_in, 1, -1).
 * Member chain: output row r (0 <= r < R) is row row0 + r of the B*S ensemble rows: it reads cond_in[(row0 + r) / S] and draws from
 *   member members_dev[r] at j = 0; 0 <= row0, row0 + R <= B*S and n_s % 4 == 0 are required; `offset` is not read.  Bit-identical to
 *   rows [row0, row0 + R) of idiff_ensemble_init given those rows' member ids (the two kernels share their body).
 * Both: state = {t0, calls0, 0} and tdev[0..R) = (float)t0 are written by one block of the same launch (no block of it reads them):
 *   the first step of the chain then runs at t0 and, in the plain chain, draws the counters offset_base + calls0*nper + v of
 *   idiff_drift_reverse_step_dev; a member chain passes calls0 = 0 (its steps draw at j = 1 + state[1]).
 *   0 < R <= 65535, t0 >= 0, calls0 >= 0; cond_in, cond, x, xa 16-byte aligned and pairwise distinct (cond_in is only read).
 *   256 threads, one float4 per lane, grid-stride; no LDS, no atomics.  A refused call (IDIFF_E_BADARG) launches nothing and leaves
 *   every buffer as it was. */
int idiff_chain_begin(const float* cond_in, float* cond, float* x, float* xa, int B, int S, int64_t n_s, int64_t row0, int R,
                      const uint64_t* members_dev, float sigma, uint64_t seed, uint64_t offset, int32_t* state, float* tdev, int t0,
                      int calls0, idiff_stream_t stream);
/* idiff_drift_reverse_step_dev (coef_rows = 3, r_prev = e_prev = NULL) or idiff_drift_reverse_step2_dev (coef_rows = 5) on R rows with
 * the z of row r drawn from member members_dev[r]'s stream at j = 1 + state[1].  Same arithmetic, order and history handling; with z_base
 * ([steps][R*n_s], indexed by state[2]) the result is bit-identical to that entry point on the same operands. */
int idiff_drift_reverse_step_members_dev(float* x, const float* r_hat, const float* e_hat, float* r_prev, float* e_prev, const float* z_base,
                                         const float* cond, float* xa, int R, int64_t n_s, const float* coef, int coef_rows, int Tp1,
                                         const int32_t* state, const uint64_t* members_dev, uint64_t seed, idiff_stream_t stream);
/* x [B][S][n_s] -> per-pixel mean [B][n_s] and sample standard deviation std [B][n_s] over the S members, fp32, members in index order:
 *   mean = (..((x_0 + x_1) + x_2)..)/S ;  std = sqrt((..((d_0^2 + d_1^2) + d_2^2)..)/(S - 1)),  d_s = x_s - mean ;  std = 0 for S = 1.
 * One rounding per operation, correctly rounded quotients and root.  A thread keeps its S values in registers between the two sums for
 * S <= 16 and reads them a second time above that (IDIFF_ENSEMBLE_REREAD=1 in the environment forces the second form; the bits are the
 * same).  The result of image b does not depend on B. */
int idiff_ensemble_stats(const float* x, float* mean, float* std_out, int B, int S, int64_t n_s, idiff_stream_t stream);
/* Per-pixel order statistics of an ensemble: x [B][S][n_s] -> out [B][nk][n_s], plane i = per pixel the ks_host[i]-th smallest
 * (0-based) of the pixel's S values.  1 <= nk <= 8; ks_host: nk host ints in [0, S), any order, duplicates allowed, passed to the kernel by
 * value (no device table).  Values are selected, never rounded: the result equals a sort of the S values, by value (which of two equal
 * values -- a signed zero -- is returned is unspecified).  If any of a pixel's S values is NaN, every plane is NaN at that pixel; +-inf
 * sort as values.  algo: 0 = auto, 1 = network form (S <= 16: the S float4 of a thread in registers, padded with +inf to 2 / 4 / 8 / 16, a
 * fixed odd-even merge sort network of v_min_f32 / v_max_f32), 2 = rank form (any S: rank_s = #{j : x_j < x_s} + #{j < s : x_j == x_s},
 * the candidate of rank ks[i] is stored; O(S^2) compares on re-read values).  Auto takes the network for S <= 16.  Both forms give the same
 * values.  n_s % 4 == 0, operands 16-byte aligned, B <= 65535, out != x; a refused call leaves the buffers untouched. */
int idiff_ensemble_order_stats(const float* x, float* out, int B, int S, int64_t n_s, const int32_t* ks_host, int nk, int algo,
                               idiff_stream_t stream);
/* Coverage of an interval map: lo, hi, target [B][n_s] -> counts [B][3] = {target < lo, lo <= target <= hi, target > hi} as exact integers.
 * A pixel where lo, hi or target is NaN counts nowhere (the three need not sum to n_s); where lo > hi nothing is inside.  Per-block partial
 * counts go to ws (idiff_interval_coverage_ws_ints(B, n_s) int32), a second launch adds them: no atomics, no float sums.
 * n_s % 4 == 0, n_s < 2^31, operands 16-byte aligned, B <= 65535. */
int idiff_interval_coverage(const float* lo, const float* hi, const float* target, int32_t* counts, int32_t* ws, int B, int64_t n_s,
                            idiff_stream_t stream);
int64_t idiff_interval_coverage_ws_ints(int B, int64_t n_s);
/* Ensemble scores: x [B][S][n_s] (the samples of an ensemble), target [B][n_s] -> per image the sums behind the CRPS and
 * the spread-skill ratio, and the rank histogram of the truth among the members.  Per pixel, members in index order s = 0 .. S-1, every
 * operation rounded once in fp32, no contraction:
 *   d_s  = x_s - y
 *   r_s  = #{ j : d_j < d_s } + #{ j < s : d_j == d_s }              a permutation of 0 .. S-1: ties take the lower rank at the lower index
 *   a    = ((|d_0| + |d_1|) + |d_2|) + ...
 *   g    = ((c_0*d_0 + c_1*d_1) + c_2*d_2) + ... ,  c_s = (float)(2 r_s - S + 1)   (exact)
 *   crps = a / S - g / S^2                                           two correctly rounded quotients, one subtraction
 *   m    = (((d_0 + d_1) + d_2) + ...) / S ;  e = m*m                squared error of the ensemble mean
 *   v    = (((d_0 - m)^2 + (d_1 - m)^2) + ...) / (S - 1) ;  v = 0 for S = 1       sample variance
 *   k    = #{ s : d_s < 0 }                                          rank of the truth, 0 .. S (= #{ x_s < y })
 * crps is the CRPS of the members' empirical CDF, (1/S) sum |x_s - y| - (1/(2 S^2)) sum sum |x_i - x_j|; since sum c_s = 0 the d_s give
 * what the x_s would in exact arithmetic, with a well-conditioned signed sum.  A member equal to the truth (d_s == 0, i.e. x_s == y) is
 * not below it, so the truth takes the lowest rank among its ties.  A pixel is invalid if any d_s is NaN: it adds to no sum and to no
 * histogram bin, is counted in `invalid`, and crps_map holds NaN there.  Infinite d_s are values: they rank and count, and make that
 * pixel's terms, and so the image's sums, non-finite.
 *   sums     float64 [B][3]    = sum crps, sum e, sum v over the valid pixels
 *   counts   int32 [B][S + 2]  = hist[0 .. S] (pixels per k), then invalid
 *   crps_map fp32 [B][n_s], or NULL to skip it
 *   ws       idiff_ensemble_scores_ws_bytes(B, S) bytes, 8-byte aligned
 * Two launches: 64 blocks per image of 256 threads, one float4 per lane per member, grid-stride; a thread adds its pixels' fp32 crps, e,
 * v into fp64 in loop order, a fixed shuffle tree per wave, the four waves in index order, one fp64 partial per block and quantity;
 * the block's histogram is S + 2 int32 bins in LDS (integer LDS adds).  The second launch adds the 64 partials of an image in index order.
 * No float atomics, no global atomics: the result of image b does not depend on B and is bit-identical from run to run.  For S <= 16 a
 * thread keeps its S float4 in registers; above that (or with IDIFF_ENSEMBLE_REREAD=1 in the environment) it takes candidates four at a
 * time and reads the members again; the bits are the same.
 * n_s % 4 == 0, n_s < 2^31, x / target / crps_map 16-byte aligned, 1 <= B <= 65535, 1 <= S <= 1024, crps_map distinct from x and target,
 * ws / sums / counts buffers of their own.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_ensemble_scores(const float* x, const float* target, float* crps_map, double* sums, int32_t* counts, void* ws, int B, int S,
                          int64_t n_s, idiff_stream_t stream);
int64_t idiff_ensemble_scores_ws_bytes(int B, int S);
/* Ensemble member distances: x [B][S][n_s] (the samples of an ensemble), target [B][n_s] or NULL -> per image the matrix of
 * squared L2 distances between whole images, and two member picks read off it.  Per image there are M = S + (target != NULL) rows
 * r_0 .. r_{M-1}: the members in index order, then the target.  A pixel is valid iff all M of its values are finite (NaN and +-inf both
 * make it invalid); an invalid pixel adds to no pair, so every entry of an image's matrix is a distance over the same pixel set.
 *   d2     float64 [B][M][M]: for i < j, d2[i][j] = d2[j][i] = sum over the valid pixels of d*d, d = (double)r_i - (double)r_j (one fp64
 *          subtraction; no Gram form: members differ by far less than their magnitude).  The diagonal is exactly +0.0 and the two
 *          halves carry the same bits.
 *   counts int32 [B][2] = {valid, invalid}
 *   pick   int32 [B][2], from the finished matrix:
 *          pick[b][0], the medoid: the first i (strict <, scanning from 0) that minimises m_i = sum_{j < S, j != i} sqrt(d2[i][j]), the
 *          correctly rounded fp64 roots added in index order; 0 for S = 1.  (With squared distances the medoid would be the member
 *          nearest to the mean; with the roots it is not.)
 *          pick[b][1], the best member: the first i that minimises d2[i][S]; -1 without a target.
 *          An image with no valid pixel has an all-zero matrix and picks 0.
 *   ws     idiff_ensemble_distances_ws_bytes(B, S, target != NULL) bytes, 8-byte aligned
 * Two launches.  The first cuts the matrix into 8 x 8 tiles: one block of 256 threads per (image, one of 64 parts, tile pair ti <= tj),
 * one float4 per lane and row, grid-stride; a thread holds its tile's 8 + 8 rows and 64 fp64 accumulators in registers (a diagonal tile
 * its 28 pairs i < j), reads the other rows too for the validity of its pixels (the re-reads across tile pairs come from L2) and folds
 * its pixels' terms into a pair's accumulator with fma(d, d, acc) in loop order, the four elements of a float4 in index order.  Then
 * idiff_ensemble_scores' reduction: a fixed xor-shuffle tree per wave (offsets 32, 16, .. 1), the four waves in index order, one fp64
 * partial per block and pair.  The second launch (one block per image) adds the 64 partials of a pair in index order and makes the
 * picks.  No atomics: the result of image b does not depend on B and is bit-identical from run to run.
 * 1 <= S <= 64, n_s % 4 == 0, n_s < 2^31, 1 <= B <= 65535; x / target 16-byte aligned, d2 / ws 8-byte aligned; d2, counts, pick and ws
 * overlap neither each other nor x or target.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_ensemble_distances(const float* x, const float* target, double* d2, int32_t* counts, int32_t* pick, void* ws, int B, int S,
                             int64_t n_s, idiff_stream_t stream);
int64_t idiff_ensemble_distances_ws_bytes(int B, int S, int has_target);
/* out [B][n_s] <- x[b][k][:] of x [B][S][n_s] with k = pick[b * pick_stride], an int32 table read on the device (no host copy): e.g. a
 * column of idiff_ensemble_distances' pick with pick_stride = 2.  A pure copy of 32-bit words in 16-byte pieces: signed zeros and NaN
 * payloads are kept.  If k is outside [0, S) the row is filled with the quiet NaN 0x7fc00000 and nothing of x is read: the table is
 * caller memory, and an out-of-range index never becomes an address.  One launch, 256 threads, grid-stride, grid = (chunks, B).
 * 1 <= S <= 64, n_s % 4 == 0, n_s < 2^31, 1 <= B <= 65535, pick_stride >= 1; x / out 16-byte aligned; out overlaps neither x nor the
 * table.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_ensemble_pick_rows(const float* x, const int32_t* pick, int pick_stride, float* out, int B, int S, int64_t n_s,
                             idiff_stream_t stream);
/* Principal modes of an ensemble: d2 [B][M][M], what idiff_ensemble_distances wrote with M = S + has_target -> per image
 * the eigen-decomposition of the members' centred Gram matrix, i.e. the PCA of the S members over the valid pixels, without another pass
 * over the images.  Only the entries i < j of d2 are read; the diagonal counts as 0.  Centring about the centroid c of the S members, for
 * all M rows, every sum in index order, every operation rounded once in fp64:
 *   a_i  = (sum_{s<S} d2[i][s]) / S ;  abar = (sum_{s<S} a_s) / S ;  h_i = a_i - abar / 2                       = |r_i - c|^2
 *   G_ij = ((h_i + h_j) - d2[i][j]) / 2                                                                          = <r_i - c, r_j - c>
 * The member block G[:S][:S] is decomposed; with a target g_s = G[S][s] and tnorm2 = h_S, the squared error of the ensemble mean.
 * Eigensolver: parallel cyclic two-sided Jacobi.  With Sp = S rounded up to even, a sweep is Sp - 1 rounds of Sp / 2 disjoint pairs by the
 * round-robin schedule of idiff_ensemble_modes_pair.  A pair p < q is rotated iff |G_pq| > 2^-53 tr0, tr0 the trace before the first sweep,
 * by Rutishauser's rotation: theta = (G_qq - G_pp) / (2 G_pq), t = sign(theta) / (|theta| + hypot(1, theta)) with sign(0) = +1,
 * c = 1 / sqrt(t^2 + 1), s = t c; a column pair (x_p, x_q) becomes (c x_p - s x_q, s x_p + c x_q), rows likewise.  Per round, a block barrier
 * between each: the rotations from the current matrix; all column updates of G and V; all row updates of G; the rotated pairs' entries
 * set to exactly 0.  The solver stops after the first sweep that rotates nothing or after 32 sweeps: the run time is bounded whatever
 * the matrix.
 *   lam    float64 [B][S]     the eigenvalues in descending order, ties by original column index (a counting rank), as computed: not clamped
 *   vec    float64 [B][S][S]  row k = the unit eigenvector of lam[k]; its component of largest magnitude is positive (the first on ties)
 *   info   int32 [B][2]       {rank, sweeps}: mode k is live iff lam[0] > 0 and lam[k] > rel_floor lam[0], rank = the live modes (at most
 *                             S - 1 in exact arithmetic); sweeps = the sweeps run, the last, idle one included, or -1 if 32 sweeps did not
 *                             end the iteration (the outputs are written all the same)
 *   coef   float64 [B][S][S]  row k = vec[k] / sqrt(lam[k]) for a live mode, zeros otherwise: u_k = sum_s coef[k][s] (x_s - c) is the mode
 *                             image, of unit L2 norm over the valid pixels (idiff_ensemble_project)
 *   tcoord float64 [B][S]     t_k = (sum_s vec[k][s] g_s) / sqrt(lam[k]) = <y - c, u_k>, fma in index order; +0.0 for a dead mode or
 *                             without a target
 *   tnorm2 float64 [B]        h_S; +0.0 without a target
 * rel_floor must lie in (0, 1).  The Python surface passes 2^-30, which sits above the error bound of idiff_ensemble_distances' matrix,
 * 2 (n + 2) 2^-53 relative for n valid pixels, only up to n of about 2^21: raise it for larger images.
 * Degenerate images are no errors: S = 1, no valid pixel or all members equal (tr0 = 0) give rank 0, sweeps 0, lam all +0.0, vec the
 * identity and coef zeros.  An image whose upper triangle holds a NaN, an infinite or a negative entry gets info = {-1, 0}, NaN in lam,
 * tcoord and tnorm2 and zeros in vec and coef; other images are untouched.
 * One launch, one block of 256 threads per image, fp64 throughout, G and V in LDS at a pitch of 65 doubles (66 560 bytes); no atomics,
 * block barriers only.  The result of image b depends on its own matrix only: not on B, its place in the batch or the run.
 * 1 <= S <= 64, 1 <= B <= 65535; every buffer 8-byte aligned, none overlapping another.  A refused call (IDIFF_E_BADARG) launches nothing
 * and leaves every buffer as it was. */
int idiff_ensemble_modes(const double* d2, int B, int S, int has_target, double rel_floor, double* lam, double* vec, double* coef,
                         double* tcoord, double* tnorm2, int32_t* info, idiff_stream_t stream);
/* The schedule idiff_ensemble_modes runs (the kernel and this entry point call one function), on the host, no GPU needed: pair i of round
 * `round` for S members.  Sp = S rounded up to even, 0 <= round < Sp - 1, 0 <= i < Sp / 2: pair 0 is (round, Sp - 1), pair i >= 1 is
 * ((round + i) mod (Sp - 1), (round - i) mod (Sp - 1)).  Returns 1 and *p < *q for a pair of members, 0 (and *p = *q = -1) for a pair that
 * touches the padding index S of an odd S, which the solver skips, IDIFF_E_BADARG outside those ranges or for a null pointer. */
int idiff_ensemble_modes_pair(int S, int round, int i, int* p, int* q);
/* x [B][S][n_s], coefficients -> out [B][K][n_s] (fp32): out[b][k] = sum_s coef_b[k][s] (x[b][s] - c), c the per-pixel mean of the S
 * members; coef_b = coef + b coef_image_stride holds K rows of S doubles (idiff_ensemble_modes' coef with stride S*S gives the K leading
 * mode images; any coefficients are taken).  Per pixel in fp64, members in index order, every operation rounded once:
 *   c = (((x_0 + x_1) + x_2) + ...) / S ;  acc_k = fma(coef[k][s], x_s - c, acc_k), acc_k = 0 at first ;  out = (float)acc_k
 * A pixel where any member is NaN or infinite gets the quiet NaN 0x7fc00000 in all K planes.  One launch, grid = (at most 64 chunks, B),
 * 256 threads, one float4 per lane and member, grid-stride; the K S coefficients go to LDS once per block (at most 4 KiB); a thread keeps
 * its S float4 in registers for S <= 16 and reads them again above that; no atomics.
 * 1 <= K <= 8, 1 <= S <= 64, 1 <= B <= 65535, n_s % 4 == 0, n_s < 2^31, coef_image_stride >= K S; x / out 16-byte aligned, coef 8-byte
 * aligned; out overlaps neither x nor the coefficients.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it
 * was. */
int idiff_ensemble_project(const float* x, const double* coef, int64_t coef_image_stride, float* out, int B, int S, int K, int64_t n_s,
                           idiff_stream_t stream);
/* Radial power spectra of image rows: x [R][H][W], sub [R / sub_rep][H][W] or NULL, bins int32 [H][Wh], Wh = W/2 + 1
 * -> out float64 [R][nb].  Row r is the plane a = x[r], or a = (double)x[r] - (double)sub[r / sub_rep] (one exact fp64 subtraction per
 * pixel: residual spectra without a temporary).  With X[u,v] = sum_y sum_x a[y,x] exp(-2 pi i (u y / H + v x / W)) and
 * P[u,v] = |X[u,v]|^2 / (H W) over 0 <= u < H, 0 <= v < Wh,
 *   out[r][k] = sum over the (u, v) with bins[u][v] == k of w_v P[u,v],   w_v = 1 for v == 0 and for v == W/2 when W is even, else 2
 * (Hermitian symmetry), so that out is the sum over the full H x W frequency plane and sum_k out[r][k] = sum a^2 (Parseval) when the
 * table sends every point to a bin.  An entry of bins outside [0, nb) drops its point: entries are compared, never used as addresses.
 * Arithmetic: fp64 throughout, the pixels widened before any operation.  The twiddle of index j and length N is the entry (j mod N) of
 * a table (cos, sin)(2 pi m / N) = sincospi(2.0 * m / N), m < N, that the first launch fills; the index is reduced in integers.  A
 * direct DFT as two GEMMs on v_mfma_f64_16x16x4_f64, the rows pass then the columns pass, one code path for any 1 <= H, W <= 1024.
 * Three launches (table; one block per strip of 16 -- H > 512: 8 -- columns v and row, which keeps the strip's rows-pass result in LDS
 * and writes w_v P to ws; one block per 64 bins and row, which adds a bin's points in a fixed order: of every 2048 points of the plane
 * in index order wave w of 16 takes the w-th 128, and the waves' sums are added in wave order).  No atomics: a row's bits depend on (H, W, bins) and its own pixels only,
 * not on R, its position among the rows or the run.  A row whose image holds a NaN or +-inf (detected, not propagated) gets the quiet
 * NaN 0x7ff8000000000000 in all nb bins; other rows are untouched.
 *   ws  idiff_radial_power_spectrum_ws_bytes(R, H, W) = 16 (W + H) + 8 ceil(R / 2) + 8 R H Wh bytes (the table, a flag per row, the
 *       weighted power planes), 8-byte aligned; 0 for sizes the call refuses
 * 1 <= R <= 65535, 1 <= H, W <= 1024, nb >= 1; with sub: sub_rep >= 1 and R % sub_rep == 0 (sub_rep is ignored without it); x, sub and
 * bins 4-byte aligned (16-byte aligned x / sub with W % 4 == 0 load in 16-byte pieces), out and ws 8-byte aligned.  A refused call
 * (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_radial_power_spectrum(const float* x, const float* sub, int sub_rep, const int32_t* bins, int nb, double* out, void* ws, int R,
                                int H, int W, idiff_stream_t stream);
int64_t idiff_radial_power_spectrum_ws_bytes(int R, int H, int W);
/* Sparsification curves of an uncertainty map: key, pred, target [B][n_s] -> per image and per point k = 0 .. K-1 of the
 * curve the error above and at the key's threshold of rank floor(k N / K), from which the host reads the error that remains after the
 * k/K most uncertain pixels are removed (models/SDEs/driftSDE.py: sparsification_summary).  Per pixel, each rounded once in fp32, no
 * contraction:
 *   d = pred - target ;  e = d*d
 * With key == NULL the ranking key is e itself (the oracle curve).  A pixel is invalid iff its key or its e is NaN: it is counted in
 * `invalid` and adds nowhere else.  +-inf keys are values and rank at the ends; an infinite e is a value and makes the sums it enters
 * non-finite.
 * Order: the key's 32 bits b become a uint32 u: 0x80000000 (-0) is first replaced by 0, in integers (no float add: denormals are
 * never touched), then u = (b >> 31) ? ~b : b | 0x80000000.  So -0 and +0 tie, denormals are distinct, and every non-NaN float has a
 * place.  With N the valid pixels of the image, for k = 0 .. K-1:
 *   m_k   = floor(k N / K), in 64-bit integers
 *   tau_k = the m_k-th largest u, counted 1-based with multiplicity
 * and for m_k = 0 (always k = 0; larger k too when N < K) the entry is the sentinel: tau = NaN (0x7fc00000), zero counts, +0.0 sums.
 *   counts int32 [B][K+1][2]    row k = {c_k = #{u > tau_k}, t_k = #{u == tau_k}};  row K = {N, invalid}
 *   sums   float64 [B][K+1][2]  row k = {A_k = sum of e over u > tau_k, T_k = sum of e over u == tau_k};  row K = {sum of e over the
 *                               valid pixels, +0.0}
 *   tau    fp32 [B][K]          the key at the threshold: the bits of the input pixel's key after the -0 -> +0 step
 *   ws     idiff_sparsification_ws_bytes(B, K, n_s) bytes, 8-byte aligned; 0 for sizes the call refuses
 * The error removed at point k is R_k = A_k + (m_k - c_k) T_k / t_k on the host: the expectation over a uniformly random order inside
 * the tie group, so the curve does not depend on how any sort would break ties (c_k < m_k <= c_k + t_k always).
 * Counts and tau are exact.  Sums are fp64 adds of the widened fp32 e in a fixed order.
 * Three launches, no sort.  (1) The selection, one block of 1024 threads per image: a most-significant-digit-first radix selection of
 * all K - 1 thresholds at once, four passes of 8 bits.  Pass 0 reads key / pred / target once, writes u (0 for an invalid pixel: no
 * valid u is 0) to ws and counts u's top byte, which also gives N; passes 1 .. 3 read u back (from L2 at the project's sizes).  Per
 * pass there is one 256-bin int32 histogram in LDS per distinct live prefix (at most 63, 63.2 KiB); the thresholds are monotone in k,
 * so a pixel finds its prefix by a binary search over the sorted prefixes, and equal prefixes share a histogram; the bins take
 * integer LDS adds (exact, the only atomics).  (2) The sums, 64 x B x ceil(K / 8) blocks of 256 threads, one float4 per lane,
 * grid-stride: a block owns eight thresholds of an image, a thread keeps their A, T, c, t in registers (one compare and one predicated
 * add each) and adds its pixels in loop order, a float4's elements in index order; then idiff_ensemble_scores' reduction, a fixed
 * xor-shuffle tree per wave, the four waves in index order, one partial per block and quantity.  (3) One block per image adds the 64
 * partials of every quantity in index order and writes the rows.  No float atomics, no global atomics: the result of image b depends
 * on its own pixels, n_s and K only, not on B, its position in the batch or the run.  A threshold read back from ws is compared,
 * never used as an address.
 * 1 <= K <= 64, 1 <= B <= 65535, n_s % 4 == 0, n_s < 2^31; key / pred / target 16-byte aligned, sums / ws 8-byte aligned; sums, counts,
 * tau and ws overlap neither each other nor the inputs.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as
 * it was. */
int idiff_sparsification(const float* key, const float* pred, const float* target, int K, double* sums, int32_t* counts, float* tau, void* ws,
                         int B, int64_t n_s, idiff_stream_t stream);
int64_t idiff_sparsification_ws_bytes(int B, int K, int64_t n_s);
/* Region-wise ensemble scores: x [B][S][n_s], target [B][n_s], labels uint8 [B][n_s] (labels_bstride = n_s) or one map
 * [n_s] shared by every image (labels_bstride = 0) -> idiff_ensemble_scores' record per region l = 0 .. L-1 of the label map.  The per-pixel
 * arithmetic is that function's contract word for word (d_s, the ranks with their tie rule, a, g, crps, m, e = m*m, v, k: every operation
 * rounded once in fp32, no contraction; a pixel is invalid if any d_s is NaN, infinite values are values); the fourth quantity is the
 * signed m itself, the mean error of the members (the region's bias).  For S = 1: crps = |d|, e = d*d, v = 0, k in {0, 1}.
 *   sums    float64 [B][L][4]     = sum crps, sum e, sum v, sum m over the valid pixels of region l
 *   counts  int32 [B][L][S + 2]   = hist[0 .. S] of region l (its valid pixels per k), then its invalid pixels
 *   outside int32 [B]             = the pixels whose label is >= L (255 is the conventional "ignore"); such a pixel adds nowhere else
 *   ws      idiff_region_scores_ws_bytes(B, S, L) bytes, 8-byte aligned
 * A label is compared against L before it is used: an out-of-range label never becomes an index.  Per image sum_l (hist + invalid) +
 * outside = n_s.
 * Two launches on idiff_ensemble_scores' order: a grid of (64, B) blocks of 256 threads; thread (p, tid) takes float4 p*256 + tid +
 * i*16384 in sweep i, with its four labels as one 32-bit load; every lane runs all ceil(n_s / 65536) sweeps (a lane past the end adds
 * nothing).  Per sweep and wave: the set of labels < L carried by a valid pixel of the wave, ascending; for each of them and each
 * quantity a lane contributes the fp64 sum of (double)term over its elements 0 .. 3 that are valid and carry the label, in element order
 * from +0.0; the wave adds these with the fixed xor tree (offsets 32, 16, .. 1); the wave's sum is added to the wave's slot [label]
 * [quantity] in sweep order; at the end the four waves' slots are added in wave order: one fp64 partial per block, label and quantity.
 * The second launch adds an image's 64 partials in index order.  Histograms are L (S + 2) int32 bins in LDS (integer LDS adds).  No float
 * atomics, no global atomics: the record of image b depends on neither B nor the run; with L = 1 and no outside label, sums[.][0][0..2]
 * carry idiff_ensemble_scores' bits for n_s <= 65536.  For S <= 16 a thread keeps its S float4 in registers; above that (or with
 * IDIFF_ENSEMBLE_REREAD=1 in the environment) it reads the members again; the bits are the same.
 * 1 <= S <= 64, 1 <= L <= 64, n_s % 4 == 0, n_s < 2^31, 1 <= B <= 65535; x / target 16-byte aligned, labels 4-byte aligned, labels_bstride
 * 0 or n_s, sums / ws 8-byte aligned; sums, counts, outside and ws overlap neither each other nor the inputs.  A refused call
 * (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_region_scores(const float* x, const float* target, const uint8_t* labels, int64_t labels_bstride, int L, double* sums,
                        int32_t* counts, int32_t* outside, void* ws, int B, int S, int64_t n_s, idiff_stream_t stream);
int64_t idiff_region_scores_ws_bytes(int B, int S, int L);
/* Intensity-band labels for idiff_region_scores: labels[i] = #{ j : edges[j] <= y[i] } (np.searchsorted(edges, y, side="right")), 255
 * where y[i] is NaN; -inf gives 0 and +inf gives ne.  1 <= ne <= 63 host floats, finite and strictly ascending, passed to the kernel by
 * value (no device table).  One launch, a thread takes 16 pixels (four 16-byte loads, one 16-byte store); a last piece shorter than
 * 16 goes element by element.  n >= 1, y and labels 16-byte aligned and not overlapping.  A refused call leaves labels untouched. */
int idiff_band_labels(const float* y, uint8_t* labels, int64_t n, const float* edges_host, int ne, idiff_stream_t stream);
/* No-reference despeckling statistics per region of a label map: x [B][S][P][H][W] (the restored rows; S = 1: one
 * restoration), ref [B][P][H][W] (the noisy input, or the target where one exists), labels uint8 [B][P][H][W] (labels_bstride = P H W) or
 * one map [P][H][W] shared by every image (labels_bstride = 0); row (b, s) uses ref[b] and labels[b].  Per pixel in fp32, every operation
 * rounded once, no contraction:
 *   a = x*scale + shift (a multiply, then an add), y likewise from ref; the pixel is valid iff a and y are both finite (unlike in
 *   idiff_region_scores +-inf is invalid: the stencils subtract);
 *   rho = y / a (correctly rounded), counted iff the pixel is valid and a >= ratio_floor;
 *   La = ((a_N + a_S) + (a_W + a_E)) - 4*a, Ly likewise, counted iff the centre and its four neighbours lie in the same H x W plane and
 *   all five are valid.  A stencil term belongs to the centre pixel's region: the neighbours' labels play no part, a neighbour with a
 *   label >= L still lends its value.
 *   sums    float64 [B][S][L][12] = sum a, a^2, y, y^2, a*y over the valid pixels of region l; sum rho, rho^2 over its ratio pixels;
 *                                   sum La, Ly, La^2, Ly^2, La*Ly over its stencil pixels.  Each term is converted to double first and
 *                                   the products are formed in double (exact: two fp32 factors), so only the summation rounds.
 *   counts  int32 [B][S][L][4]    = the region's valid, ratio, stencil and invalid pixels
 *   outside int32 [B]             = the pixels whose label is >= L (255 is the conventional "ignore"); such a pixel adds nowhere else
 *   ws      idiff_despeckle_stats_ws_bytes(B, S, L) bytes, 8-byte aligned
 * A label is compared against L before it is used: an out-of-range label never becomes an index.  Per row sum_l (valid + invalid) +
 * outside = P H W.  H <= 2 leaves no stencil pixel: those counts are 0 and those sums +0.0.
 * Two launches on idiff_region_scores' order: a grid of (64, B S) blocks of 256 threads; thread (p, tid) of a row takes the aligned
 * float4 p*256 + tid + i*16384 of the row's P H W / 4 in sweep i (W % 4 == 0: a float4 never spans two lines), its four labels as one
 * 32-bit load, its N / S neighbours as the aligned float4 one line up / down and the W / E neighbours of its end elements as two scalar
 * loads, all from global memory and only where they lie in the centre's plane; every lane runs all ceil(P H W / 65536) sweeps (a lane
 * past the end adds nothing).  Per sweep and wave: the set of labels < L carried by a valid pixel of the wave, ascending; for each of
 * them and each quantity in the order above a lane contributes the fp64 sum of the terms of its elements 0 .. 3 that carry the label and
 * count for the quantity, in element order from +0.0; the wave adds these with the fixed xor tree (offsets 32, 16, .. 1); the wave's sum
 * is added to the wave's slot [label][quantity] in sweep order; at the end the four waves' slots are added in wave order: one fp64
 * partial per block, label and quantity.  The second launch adds a row's 64 partials in index order.  Counts are L * 4 int32 in LDS
 * (integer LDS adds).  No float atomics, no global atomics: the record of row (b, s) depends on neither B, S, the other rows nor the run.
 * 1 <= S <= 64, 1 <= L <= 64, W % 4 == 0, P H W < 2^31, B S <= 65535; scale and shift finite, ratio_floor finite and > 0; x / ref 16-byte
 * aligned, labels 4-byte aligned, labels_bstride 0 or P H W, sums / ws 8-byte aligned; sums, counts, outside and ws overlap neither each
 * other nor the inputs.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_despeckle_stats(const float* x, const float* ref, const uint8_t* labels, int64_t labels_bstride, int L, float scale, float shift,
                          float ratio_floor, double* sums, int32_t* counts, int32_t* outside, void* ws, int B, int S, int P, int H, int W,
                          idiff_stream_t stream);
int64_t idiff_despeckle_stats_ws_bytes(int B, int S, int L);
/* Flips and transpositions of image rows (driftSDE self_ensemble): in [R / in_rep][C][H][W] -> out [R][C][H][W].  Row r reads
 * input row r / in_rep under the 3-bit code k = (codes >> 3*((r % S) % period)) & 7: bit 0 = transpose, bit 1 = flip H, bit 2 = flip W,
 * the flips applied after the transposition:
 *   y1 = bit1 ? H-1-y : y ;  x1 = bit2 ? W-1-x : x ;  out[r,c,y,x] = bit0 ? src[c,x1,y1] : src[c,y1,x1]
 * (in torch terms: x.transpose(-1,-2) if bit 0, then .flip(-2) if bit 1, then .flip(-1) if bit 2).  The up to 8 codes travel by value, 3
 * bits each from bit 0 up; there is no device table.  A code without bit 0 is its own inverse; the inverse of a code with bit 0 has
 * bits 1 and 2 swapped.  The host computes inverses: the kernel has no inverse mode.
 * A pure permutation of 32-bit words: bit-identical to the expression above, signed zeros and NaN payloads included.
 * One launch, grid = (64x64 output tiles of a plane, C, R), 256 threads: a non-transposing row moves 16-byte pieces from the mirrored
 * position (words reversed under bit 2) without LDS; a transposing row stages its tile in LDS at a pitch of 65 dwords, 16-byte loads along
 * the input's W and 16-byte stores along the output's W.  Offsets are 64-bit.
 * Required: 1 <= period <= 8, S >= 1, in_rep >= 1, R >= 1, R % in_rep == 0, C >= 1, H >= 1, W % 4 == 0, H == W if any of the `period` codes has
 * bit 0 set, R <= 65535 and C <= 65535 (grid axes), in and out 16-byte aligned and not overlapping.  A refused call (IDIFF_E_BADARG)
 * launches nothing and leaves every buffer as it was. */
int idiff_dihedral_rows(const float* in, float* out, int R, int C, int H, int W, int in_rep, int S, int period, uint32_t codes,
                        idiff_stream_t stream);
/* ---- tiled sampling (driftSDE tile / tile_overlap) ----
 * The chain's state is one full-resolution image [B][C][H][W]; the nets see it as a batch of ny*nx windows of Ph x Pw per image, window
 * row ((b*ny + iy)*nx + ix), each [C][Ph][Pw] contiguous.  W, Pw and the W origins are multiples of 4; all operands 16-byte aligned.
 * The host plan (models/SDEs/driftSDE.py, tile_plan) hands in two tables per axis of length L with n windows, on the device:
 *   ytab / xtab  int32 [3*L + n] = first[L] | cov_lo[L] | cov_hi[L] | origin[n]
 *   ywt  / xwt   fp32  [2*L]     = w0[L] | w1[L]
 * first[c]: the lower of the at most two (adjacent) windows with non-zero blend weight at coordinate c; w0[c] / w1[c]: the weights of
 * windows first[c] and first[c] + 1 (exactly 1 and 0 outside the blend zones); windows cov_lo[c] <= i < cov_hi[c] are those whose extent
 * [origin[i], origin[i] + P) holds c.  The entry points check the sizes; the table contents are the plan's responsibility.
 * tiles[row, c, :, :] = full[b, c, origin_y[iy] : +Ph, origin_x[ix] : +Pw]  (reads ytab / xtab's origins only) */
int idiff_tile_gather(const float* full, float* tiles, int B, int C, int H, int W, int ny, int nx, int Ph, int Pw, const int32_t* ytab,
                      const int32_t* xtab, idiff_stream_t stream);
/* The step of a tiled chain, per pixel of the full image, per-step scalars from coef / state as in idiff_drift_reverse_step_dev:
 *   R^ = blend of r_tiles over the slots (iy0, ix0), (iy0, ix1), (iy1, ix0), (iy1, ix1) in that order, iy0 = first_y, iy1 = iy0 + 1 (x alike):
 *        w = wy*wx (one fp32 product);  acc = w*r for the first term, acc = acc + w*r after it;  a slot whose w is exactly 0 is skipped and
 *        its memory is not read, so a singly covered pixel is 1.0f*r, exact.   e^ likewise from e_tiles.
 *   coef_rows = 5: r_prev / e_prev [B][C][H][W] hold the previous jump's BLENDED predictions; the extrapolation, its zero-rho rule and the
 *        hand-over (r_prev <- R^, e_prev <- e^) are idiff_drift_reverse_step2_dev's.  coef_rows = 3: r_prev = e_prev = NULL.
 *   z  = z_base[state[2]][v] (injected, full image) or the Philox normals of counter offset_base + state[1]*nper + v, v the float4 index
 *        in the flattened full image: the counter of idiff_drift_reverse_step_dev on that image, whatever the tiling.
 *   x <- ((x - a*R^) - b*e^) + c*z ;  xa = x - cond ;  x and xa are then written into x_tiles / xa_tiles of every window whose extent
 *        holds the pixel (by extent, not by weight: a window's border is filled where its weight is 0).
 * With one window per pixel the full-image x is bit-identical to idiff_drift_reverse_step_dev / _step2_dev on the gathered operands. */
int idiff_drift_reverse_step_tiled_dev(float* x, const float* r_tiles, const float* e_tiles, float* r_prev, float* e_prev, const float* z_base,
                                       const float* cond, float* x_tiles, float* xa_tiles, int B, int C, int H, int W, int ny, int nx, int Ph,
                                       int Pw, const int32_t* ytab, const float* ywt, const int32_t* xtab, const float* xwt, const float* coef,
                                       int coef_rows, int Tp1, const int32_t* state, uint64_t seed, uint64_t nper, uint64_t offset_base,
                                       idiff_stream_t stream);
/* The step of a tiled chain on the rows of a posterior ensemble (driftSDE tiled_ensemble).  x, cond, r_prev, e_prev are R
 * full-resolution rows [R][C][H][W], row r one member of one input image (cond per row, as idiff_ensemble_init writes cond_rep); the
 * window buffers hold row ((r*ny + iy)*nx + ix): idiff_drift_reverse_step_tiled_dev's geometry with B = R.  Per float4 group v of row r
 * (Q = C*H*W/4 groups per row) the blend, the extrapolation and its zero-rho rule, the update, the hand-over and the scatter are those of
 * idiff_drift_reverse_step_tiled_dev (one kernel template, one copy of each piece); only z differs:
 *   z  = z_base[state[2]][r*Q + v] (injected, [steps][R*C*H*W]) or the Philox normals of counter (1 + state[1])*Q + v under member
 *        members_dev[r]: the draw idiff_drift_reverse_step_members_dev and idiff_randn_members(j = 1 + state[1]) give that member for a
 *        sample of n_s = C*H*W, whatever the tiling and whatever rows sit beside it.  Nothing is drawn or read where c == 0.
 * Bit-identity contracts: (1) with z_base, or with device noise against z_base = idiff_randn_members(j = 1 + state[1]), every output
 * (x, x_tiles, xa_tiles, r_prev, e_prev) equals idiff_drift_reverse_step_tiled_dev's at B = R on the same operands; (2) with one window
 * (ny = nx = 1, Ph = H, Pw = W) x and xa_tiles equal x and xa of idiff_drift_reverse_step_members_dev on the same operands.
 * 256 threads, one float4 per lane, grid-stride, grid = (chunks, R); no LDS, no atomics.  Every size and alias check of
 * idiff_drift_reverse_step_tiled_dev holds with R in place of B, and 0 < R <= 65535, members_dev != NULL, W % 4 == 0, all operands 16-byte
 * aligned.  A refused call (IDIFF_E_BADARG) launches nothing and leaves every buffer as it was. */
int idiff_drift_reverse_step_tiled_members_dev(float* x, const float* r_tiles, const float* e_tiles, float* r_prev, float* e_prev,
                                               const float* z_base, const float* cond, float* x_tiles, float* xa_tiles, int R, int C, int H,
                                               int W, int ny, int nx, int Ph, int Pw, const int32_t* ytab, const float* ywt,
                                               const int32_t* xtab, const float* xwt, const float* coef, int coef_rows, int Tp1,
                                               const int32_t* state, const uint64_t* members_dev, uint64_t seed, idiff_stream_t stream);
/* t <- t-1 (back to T once t <= t_stop), both counters += 1, tdev[0..B) = (float)t   (the UNets' timestep input) */
int idiff_step_state_advance(int32_t* state, float* tdev, int B, int T, int t_stop, idiff_stream_t stream);
/* Few-step schedule form (driftSDE sample_T / sample_timesteps): t <- next_t[t] (back to t_first once t <= t_stop), both counters += 1,
 * tdev[0..B) = (float)t.  next_t int32[Tp1] maps each schedule point t_k to t_{k+1}; a t outside [0, Tp1) restarts at t_first, so
 * next_t is never read out of bounds.  The coef rows of idiff_drift_reverse_step_dev are then the jump coefficients t_k -> t_{k+1}. */
int idiff_step_state_advance_table(int32_t* state, float* tdev, int B, const int32_t* next_t, int Tp1, int t_first, int t_stop,
                                   idiff_stream_t stream);
/* Inverted dropout (training mode of the ScoreMapModule decoder blocks: nn.Dropout(0.1) in TransformerDecoderLayer / Attention.proj_drop,
 * models/_modified_BiomedCLIP.py:448-478,520-549): out[i] = x[i] / (1-p) where u_i >= p, else 0, with u_i = (w >> 8) * 2^-24 from word
 * i % 4 of Philox counter offset + i / 4 under `seed`.  The mask is a function of (seed, offset, i) alone: the backward pass is the SAME
 * call on the gradient (nothing is stored), x == out allowed. */
int idiff_dropout(const float* x, float* out, int64_t n, float p, uint64_t seed, uint64_t offset, idiff_stream_t stream);
/* standard normals (Philox4x32-10, Box-Muller), element i uses counter (offset + i/4) lane i%4 */
int idiff_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, idiff_stream_t stream);
/* raw Philox4x32-10 words for tests: out[4*i..4*i+3] = philox(counter = offset+i, key = seed) */
int idiff_philox_raw(uint32_t* out, int64_t ncounters, uint64_t seed, uint64_t offset, idiff_stream_t stream);
/* out = alpha*x + beta*y */
int idiff_axpby(const float* x, const float* y, float* out, int64_t n, float alpha, float beta, idiff_stream_t stream);
/* Gradient fan-in in one pass: out[b, :] = srcs[0][b, :] + srcs[1][b, :] (+ ..), 2..4 sources with their own batch strides (a source may
 * be a channel slice of a bigger tensor), summed in argument order.  Replaces torch.autograd's pairwise accumulation (n - 1 passes
 * plus a copy per non-contiguous operand) where a feature map has several consumers.  per_sample % 4 == 0, 16-byte aligned rows. */
int idiff_sum_n(const float* const* srcs, const int64_t* src_bstrides, int nsrc, float* out, int64_t out_bstride, int B,
                int64_t per_sample, idiff_stream_t stream);
/* Many tensors -> one flat buffer in one launch (replaces the per-parameter gradient accumulate / copy launches of
 * torch.autograd's AccumulateGrad + optimizer packing; models/drift_noise_model.py:292-296 semantics unchanged).  segs_dev: device
 * array of nseg records {const float* src (NULL = zero fill); int64 dst_offset; int64 n; int64 first_block}, first_block = running
 * sum of ceil(n / 4096), ascending; nblocks = its total. */
int idiff_gather_segments(const void* segs_dev, int nseg, int64_t nblocks, float* dst, idiff_stream_t stream);
/* The accumulating form, for gradient accumulation (FusedAdam accum_steps > 1: micro-batches 2..k of a group): same table, same
 * block mapping, dst[dst_offset + i] = dst[dst_offset + i] + src[i] -- one fp32 add, each element owned by one thread (no atomics:
 * the result is a function of the operands alone).  A record with src == NULL leaves its range of dst untouched (the assigning
 * entry point zero-fills it); so does everything between the records. */
int idiff_gather_segments_acc(const void* segs_dev, int nseg, int64_t nblocks, float* dst, idiff_stream_t stream);
/* forward marginals with per-sample coefficients (training-state samplers):
 *   out[b,:] = c0[b]*x0[b,:] + c1[b]*cond[b,:] + c2[b]*eps[b,:]      (driftSDE.forward_diffusion, IRSDE.generate_random_states) */
int idiff_mix3_per_sample(const float* x0, const float* cond, const float* eps, const float* c0, const float* c1,
                          const float* c2, float* out, int B, int64_t per_sample, idiff_stream_t stream);

/* ================================================================================================
 * TRAINING PATH (models/drift_noise_model.py:242-312: loss.backward() + Adam).  The reference gets its
 * backward from ATen autograd; here every gradient kernel is explicit.
 * ============================================================================================== */

/* Weight gradient of idiff_conv2d_fwd for the SAME descriptor (sources, mode, ks, prologue are re-gathered the
 * way the forward gathered them; wpk/bias/out/epilogue fields are ignored):
 *   dw[co][ci][ky][kx] (torch layout) (+)= sum_{b,y,x} dy[b,co,y,x] * X[b,ci,y+ky-p,x+kx-p]
 * ws: workspace of idiff_conv2d_wgrad_ws_floats(d) floats (per-split partials, reduced in a fixed order). */
int64_t idiff_conv2d_wgrad_ws_floats(const idiff_conv_desc* d);
int idiff_conv2d_wgrad(const idiff_conv_desc* d, const float* dy, int64_t dy_bstride, float* dw, int accumulate, float* ws,
                       idiff_stream_t stream);
/* With d->operands == 1 an eligible 3x3 layer (the shapes of IDIFF_CONV_ALGO_BF16) takes the bf16-operand form:
 *   dW = sum bf16(dY) * bf16(X~), summed in fp32; per-(sample, block of up to 16 8x32 patches) partials reduced in sample / block order,
 *   no atomics: bitwise reproducible, independent of the grid.  last_algo = IDIFF_CONV_ALGO_BF16. */
/* IDIFF_CONV_ALGO_* of the calling thread's last idiff_conv2d_wgrad: the Winograd form (conv_wino_wgrad.hip) takes 3x3
 * layers with Cout % 64 == 0, Cin % 16 == 0 (C0 % 64 == 0 with a second source), Hout % 2 == 0, Wout % 16 == 0 */
int idiff_conv2d_wgrad_last_algo(void);
/* data-gradient helpers: the data gradient itself is idiff_conv2d_fwd on dy with idiff_pack_conv_weight_T weights */
int idiff_sumpool2x2(const float* x, float* out, int64_t planes, int h, int w, idiff_stream_t stream);     /* upsample^T   */
int idiff_pixel_shuffle2(const float* x, float* out, int B, int C, int h, int w, idiff_stream_t stream);    /* unshuffle^T  */
/* out_bc[b*C+c] = sum_p x[b,c,p];  out_c[c] (+)= sum_b in_bc[b*C+c]   (bias / per-(b,c) vector gradients) */
int idiff_plane_sum(const float* x, int64_t x_bstride, float* out_bc, int B, int C, int HW, idiff_stream_t stream);
int idiff_batch_sum(const float* in_bc, float* out_c, int B, int C, int accumulate, idiff_stream_t stream);

/* Backward of y = silu(a[b,c]*h + b[b,c]) with (a,b) = idiff_gn_finalize(stats(h), gamma, beta, film): gradient
 * w.r.t. h THROUGH the GroupNorm statistics, dgamma/dbeta [C], dfilm [B,2C] (scale | shift).  a, b, mean_rstd as
 * produced by idiff_gn_finalize.  ws: idiff_gn_silu_bwd_ws_floats(B,C,groups) floats.  Optional, from the same reads (no pass of
 * their own): dh_sum [C] = sum over samples and pixels of dh (the bias gradient of the conv that produced h), dy_sum [B,C] = sum
 * over pixels of dy (the gradient of a per-(sample, channel) vector added behind the activation); NULL = not wanted. */
int64_t idiff_gn_silu_bwd_ws_floats(int B, int C, int groups);
int idiff_gn_silu_bwd(const float* dy, int64_t dy_bstride, const float* h, int64_t h_bstride, const float* a, const float* b,
                      const float* mean_rstd, const float* gamma, const float* beta, const float* film, int64_t film_ld,
                      float* dh, int64_t dh_bstride, float* dgamma, float* dbeta, float* dfilm, int64_t dfilm_ld, float* ws,
                      int B, int C, int groups, int HW, int accumulate, float* dh_sum, float* dy_sum, idiff_stream_t stream);

/* elementwise activations (token side) and their gradients: dx = dy * act'(x) */
int idiff_act_fwd(const float* x, float* y, int64_t n, int act, idiff_stream_t stream);
int idiff_act_bwd(const float* dy, const float* x, float* dx, int64_t n, int act, idiff_stream_t stream);
/* out[n] (+)= sum_r x[r,n]  (Linear bias gradient) */
int idiff_colsum(const float* x, int64_t ldx, float* out, int R, int N, int accumulate, idiff_stream_t stream);
/* out[r,n] = x[r,n]*g[n]  and  out[n] = sum_r x[r,n]*y[r,n]  (dense [R,N]; ScoreMapModule gamma and its gradient) */
int idiff_scale_cols(const float* x, const float* g, float* out, int R, int N, idiff_stream_t stream);
int idiff_colsum_prod(const float* x, const float* y, float* out, int R, int N, idiff_stream_t stream);
/* Grouped forms for STACKED token matrices (r05: the same layer of a net's four ScoreMapModule decoders as one [groups * Rg, .] matrix):
 * R rows in `groups` equal groups, each with its own parameter / output row -- gamma, beta, dgamma, dbeta [groups][C]; out [groups][N]. */
int idiff_layernorm_rows_g_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out, int64_t ldo, int R, int C,
                               float eps, float* mean_rstd, int groups, idiff_stream_t stream);
int idiff_layernorm_rows_g_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, const float* mean_rstd,
                               float* dx, int64_t lddx, float* dgamma, float* dbeta, int R, int C, int groups, idiff_stream_t stream);
int idiff_colsum_g(const float* x, int64_t ldx, float* out, int R, int N, int groups, idiff_stream_t stream);
int idiff_layernorm_rows_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                             const float* mean_rstd, float* dx, int64_t lddx, float* dgamma, float* dbeta, int R, int C,
                             int accumulate, idiff_stream_t stream);
/* ws: idiff_chan_layernorm_bwd_ws_floats(B, C, HW) floats (>= 2*B*C): per-(sample, workgroup, channel) partials of dgamma / dbeta,
 * reduced in a fixed order; dx and the partials come out of ONE pass over dy and x (C <= 256) */
int64_t idiff_chan_layernorm_bwd_ws_floats(int B, int C, int HW);
int idiff_chan_layernorm_bwd(const float* dy, int64_t dy_bstride, const float* x, int64_t x_bstride, const float* gamma,
                             const float* mean_rstd, float* dx, int64_t dx_bstride, float* dgamma, float* dbeta, float* ws,
                             int B, int C, int HW, int accumulate, idiff_stream_t stream);
/* y = x / max(|x|_2 over channels, 1e-12) per pixel (F.normalize(dim=1)); nrm [B,HW] */
int idiff_chan_normalize_fwd(const float* x, int64_t x_bstride, float* y, float* nrm, int B, int C, int HW,
                             idiff_stream_t stream);
int idiff_chan_normalize_bwd(const float* dy, const float* y, const float* nrm, float* dx, int64_t dx_bstride, int B, int C,
                             int HW, idiff_stream_t stream);
/* out[b, idx[b], p] = x[b,0,p], zeros elsewhere (gradient of idiff_gather_channel) */
int idiff_scatter_channel(const float* x, const int32_t* idx, float* out, int B, int C, int HW, idiff_stream_t stream);

/* generic batched GEMM on the f32 matrix cores:  C[b] = alpha * op(A[b]) (MxK) . op(B[b]) (KxN) + beta * C[b]
 * (row-major; transX != 0 -> the matrix is stored transposed); sA/sB/sC = batch strides in elements */
int64_t idiff_bgemm_ws_floats(int M, int N, int K, int batch); /* 0 unless the shape is K-split (long K, tiny output) */
int idiff_bgemm(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                int transA, int transB, int64_t sA, int64_t sB, int64_t sC, int batch, float alpha, float beta, float* ws,
                idiff_stream_t stream);
/* the same with a per-column bias per batch entry (colbias [batch][N] with batch stride sbias, or NULL), beta = 0, no K split */
int idiff_bgemm_bias(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int transA,
                     int transB, int64_t sA, int64_t sB, int64_t sC, int batch, float alpha, const float* colbias, int64_t sbias,
                     idiff_stream_t stream);
/* y [R,N] = x [R,K] . w [N,K]^T (+ bias [N] or NULL) through the same kernel: the training path's token-side linear layers
 * (reference: nn.Linear inside TransformerDecoderLayer / ContextDecoder, models/modules/_modified_BiomedCLIP.py); any R */
int idiff_linear_mfma_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* out, int64_t ldo, int R,
                          int K, int N, idiff_stream_t stream);
/* out = softmax(scale * x) over each row;  ds = scale * p * (dp - <p, dp>) */
int idiff_softmax_rows_fwd(const float* x, int64_t ldx, float* out, int64_t ldo, int R, int N, float scale,
                           idiff_stream_t stream);
int idiff_softmax_rows_bwd(const float* p, int64_t ldp, const float* dp, int64_t lddp, float* ds, int64_t ldds, int R, int N,
                           float scale, idiff_stream_t stream);

/* losses (drift_noise_model.py:234-240,270,279): bilinear resize of the label (align_corners=False, no antialias;
 * torchvision Resize is unpinned in the reference) and mean squared error with its gradient
 * grad = grad_scale * 2 (a-b) / n  (grad may be NULL); ws: 256 floats; loss: 1 float on the device */
int idiff_resize_bilinear(const float* x, float* out, int64_t planes, int H, int W, int oh, int ow, idiff_stream_t stream);
int idiff_mse_loss(const float* a, const float* b, float* loss, float* grad, float* ws, int64_t n, float grad_scale,
                   idiff_stream_t stream);
/* validation metrics of the drivers (trainUM.py:314-329, testUM.py:151-164) on x/2+0.5, data_range 1:
 * out_b3[b] = {RMSE, PSNR dB, SSIM (skimage: gaussian 11x11 sigma 1.5, K1 .01, K2 .03, interior crop)};
 * pred/target [B,H,W]; ws: B*128 floats.
 * SSIM is NaN, not 0, for H < 11 or W < 11 (no pixel has a whole window; skimage refuses such an image); RMSE and PSNR are as ever.
 * Operation order, fp32: per interior pixel the five window moments are accumulated on values shifted by the window-centre pixels,
 * da = 0.5 (p - p0), dc = 0.5 (t - t0) (sum w da, sum w dc, sum w da^2, sum w dc^2, sum w da dc; the variances and the covariance are
 * shift-invariant, the means get (0.5 p0 + 0.5), (0.5 t0 + 0.5) added back), so a locally flat bright or saturated region does not
 * cancel against C2 = 9e-4 as raw moments sum w a^2 - (sum w a)^2 do; the final quotient runs without FMA contraction, so pred ==
 * target gives exactly 1.  Pixel values are summed by thread i of 64 x 256 over pixels i, i + 16384, ..., a 64-lane butterfly, the four
 * waves of a workgroup in order, and the 64 partials of an image in fp64.  A null pointer or B, H or W < 1: IDIFF_E_BADARG, nothing
 * launched. */
int idiff_image_metrics(const float* pred, const float* target, float* out_b3, float* ws, int B, int H, int W,
                        idiff_stream_t stream);
/* torch.optim.Adam semantics (L2-in-gradient weight decay, config.yml:138-143), grad pre-scaled by grad_scale
 * (1/world after the flat RCCL all-reduce); step >= 1 */
int idiff_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float grad_scale, int step, idiff_stream_t stream);

/* Gradient-norm guard of the optimizer step (global-norm clipping as torch.nn.utils.clip_grad_norm_, and skipping a step whose
 * gradient is not finite; the reference's loop has neither).  Three launches back to back on one stream, nothing read on the host.
 *
 * idiff_grad_sumsq: part[k] = sum of g[i]^2 over the elements workgroup k owns, k < P = idiff_grad_sumsq_parts() = 1024 (a fixed
 * grid of P workgroups x 256 threads, four per CU).  A thread strides over the float4s of g with the whole grid, keeps one fp32
 * accumulator per float4 lane and adds them as (x + y) + (z + w); wave sums, then the four wave sums through LDS as
 * (w0 + w1) + (w2 + w3); the n % 4 tail elements go, one by one, to thread 0 of workgroup 0; a workgroup with no element writes 0.
 * No atomics, nothing passed between workgroups: part is a function of (g, n) alone, bit-identical from run to run.
 * g: 16-byte aligned; n >= 1.  A misaligned g, n < 1 or a null pointer: IDIFF_E_BADARG, nothing launched, part untouched. */
int64_t idiff_grad_sumsq_parts(void);
int idiff_grad_sumsq(const float* g, int64_t n, float* part /* [P] */, idiff_stream_t stream);
/* idiff_grad_guard: one wave over the nbuf * P partials of nbuf >= 1 buffers (each buffer's idiff_grad_sumsq wrote its own range
 * [b * P, (b + 1) * P) of part: one norm over all parameter groups).  Lane l adds part[l], part[l + 64], ... in index order in fp64,
 * the 64 lane sums meet in a fixed butterfly: S.  info [4] on the device:
 *   info[0] = norm    = (float)(|grad_scale| * sqrt(S)), in fp64, rounded once: the L2 norm of the gradient as idiff_adam_step scales it
 *   info[1] = coef    = 1 if max_norm <= 0 (no clipping), else (float)min(1, max_norm / ((double)norm + 1e-6)): clip_grad_norm_ with
 *                       error_if_nonfinite=False -- an inf norm gives 0, a NaN norm gives NaN
 *   info[2] = applied = 0.0f if skip_nonfinite != 0 and norm is NaN or +-inf, else 1.0f.  The partials are fp32: a sum of squares
 *                       that overflows fp32 (or a norm that overflows it) is inf and counts as non-finite
 *   info[3] = 0 */
int idiff_grad_guard(const float* part, int nbuf, float grad_scale, float max_norm, int skip_nonfinite, float* info /* [4] */,
                     idiff_stream_t stream);
/* idiff_adam_step with coef = info[1] and applied = info[2] read on the device (uniform over the grid).  applied == 0: every thread
 * returns before it reads or writes p, m or v, which stay bit for bit as they were whatever g holds.  Otherwise the gradient is
 * (g[i] * grad_scale) * coef and the rest is idiff_adam_step's update, the same device code; with coef == 1.0f the result is
 * bit-identical to idiff_adam_step on the same operands.  info must not overlap p, g, m or v (IDIFF_E_BADARG). */
int idiff_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float grad_scale, int step, const float* info, idiff_stream_t stream);

/* bf16 wire format of the data-parallel gradient exchange (replaces nothing in the reference, whose DDP buckets are fp32,
 * models/drift_noise_model.py:145-146; BASELINE config c3 asks for it): round-to-nearest-even pack of the flat fp32 gradient
 * buffer, and the widening unpack after the all-reduce.  The fp32 buffer stays the master copy Adam reads. */
int idiff_f32_to_bf16(const float* x, uint16_t* out, int64_t n, idiff_stream_t stream);
int idiff_bf16_to_f32(const uint16_t* x, float* out, int64_t n, idiff_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IDIFF_H */
