// Radial power spectra of image rows (include/idiff.h: idiff_radial_power_spectrum).  Row r is the H x W plane x[r], or
// (double)x[r] - (double)sub[r / sub_rep]; its 2-D DFT X[u, v] over the half plane 0 <= v < Wh = W/2 + 1 gives P = |X|^2 / (H W), and
// out[r][k] adds w_v P over the points whose entry of the caller's table `bins` is k.  A direct DFT as two GEMMs in fp64 on
// v_mfma_f64_16x16x4_f64: one code path for any 1 <= H, W <= 1024.
//
// Three launches.
//   1. spectrum_twiddle_kernel fills the table tab[j] = (cos, sin)(2 pi j / N) for j < N, N = W then N = H, with sincospi(2.0 * j / N).
//      Every twiddle of the transform is an entry of it at an index reduced in integers, (j k) mod N.
//   2. spectrum_dft_kernel, one block of 4 waves per (strip of sv columns v, row).  Rows pass: Y[y, v] = sum_x a[y, x] e^{-2 pi i x v / W}
//      for all y and the strip's v, the pixels widened to fp64 as the A operand and the table as B; Y stays in LDS as two planes
//      [H][sv].  Columns pass: X[u, v] = sum_y e^{-2 pi i u y / H} Y[y, v], the table as A and the LDS planes as B, four real MFMAs per
//      k-step; the epilogue writes w_v |X|^2 / (H W) to the workspace.  sv = 16 for H <= 512 and 8 above it (the planes then still fit
//      the LDS of a CU; the other eight columns of the tile are zeros).  Tiles past an edge take zeros for what lies outside the
//      operands and are not written.  Every block reads its whole row image, so each one knows by itself whether it is finite.
//      The kernel has no static LDS: its dynamic block is all it takes, 160 KB at H = W = 1024.
//   3. spectrum_bin_kernel, one block of 16 waves per (64 bins, row): lane l owns bin k.  The plane's H * Wh points are taken in index
//      order in pieces of 16 x 128; wave w adds, in index order, the points of the w-th 128 of every piece whose table entry equals k
//      (a compare: the entry never becomes an address), then the 16 waves' sums are added in wave order.  The block stages a piece of
//      the table and the plane in LDS; a wave reads its part from there as broadcasts.  No atomics; the order depends on (H, W, bins)
//      alone.
#include "common.h"

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int SPEC_MAX_N = 1024;
constexpr int SPEC_BIN_WAVES = 16;
constexpr int SPEC_BIN_CHUNK = 128;  // points of a line staged at a time
constexpr unsigned long long QNAN64_BITS = 0x7ff8000000000000ull;

__host__ __device__ inline int spec_strip(int H) { return H <= 512 ? 16 : 8; }

// The one statement of the workspace: the twiddle table, a flag per row, the weighted power plane of every row.
struct spec_ws {
    int64_t tab, flags, power, total;  // byte offsets, and the size
};
inline spec_ws spec_ws_layout(int R, int H, int W) {
    spec_ws l;
    l.tab = 0;
    l.flags = l.tab + 16ll * (W + H);
    l.power = l.flags + 8ll * ((R + 1) / 2);
    l.total = l.power + 8ll * R * H * (W / 2 + 1);
    return l;
}

__global__ __launch_bounds__(256) void spectrum_twiddle_kernel(double2* __restrict__ tab, int W, int H) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W + H) return;
    const int N = j < W ? W : H, m = j < W ? j : j - W;  // 0 <= m < N: the index is reduced already
    double s, c;
    sincospi(2.0 * (double)m / (double)N, &s, &c);
    tab[j] = make_double2(c, s);
}

// a[e] = the row image at (y, x + e), e = 0 .. 3, as fp64; 0 outside the image.  `vec`: W % 4 == 0 and 16-byte aligned bases.
__device__ __forceinline__ void spec_load4(const float* __restrict__ img, const float* __restrict__ sb, int y, int x, int H, int W, bool vec,
                                           double (&a)[4], bool& bad) {
    float f[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
    if (y < H && x < W) {
        const long long o = (long long)y * W + x;
        if (vec) {
            const floatx4 t = *reinterpret_cast<const floatx4*>(img + o);
            f[0] = t[0], f[1] = t[1], f[2] = t[2], f[3] = t[3];
            if (sb) {
                const floatx4 q = *reinterpret_cast<const floatx4*>(sb + o);
                g[0] = q[0], g[1] = q[1], g[2] = q[2], g[3] = q[3];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) {
                    f[e] = img[o + e];
                    if (sb) g[e] = sb[o + e];
                }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] = __dsub_rn((double)f[e], (double)g[e]);
        bad |= !(fabs(a[e]) < __builtin_inf());
    }
}

__device__ __forceinline__ doublex4 mfma64(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Two waves per SIMD (two blocks per CU at H <= 256): without the bound the compiler spreads over 470 registers and one block runs alone.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void spectrum_dft_kernel(
    const float* __restrict__ x, const float* __restrict__ sub, int sub_rep, const double2* __restrict__ tab, int32_t* __restrict__ flags,
    double* __restrict__ power, int H, int W, int vec) {
    extern __shared__ double2 spec_lds[];
    const int sv = spec_strip(H), Wh = W / 2 + 1;
    double2* twW = spec_lds;  // [W], then [H]
    double2* twH = spec_lds + W;
    double* Yr = reinterpret_cast<double*>(spec_lds + W + H);  // [H][sv]
    double* Yi = Yr + H * sv;
    const long long r = blockIdx.y;
    const int v0 = blockIdx.x * sv;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    const float* img = x + r * H * W;
    const float* sb = sub ? sub + (r / sub_rep) * H * W : nullptr;
    for (int j = threadIdx.x; j < W + H; j += blockDim.x) spec_lds[j] = tab[j];
    __syncthreads();
    const int ntile = (H + 15) / 16;
    bool bad = false;

    // rows pass: A = the image [y][x], B = e^{-2 pi i x v / W} [x][v].  Within a chunk of 16 x, k-step s of lane group lg takes
    // x = x0 + 4 lg + s, so that a lane's four steps come from one 16-byte load.
    {
        const int v = v0 + li;
        int idx[4], step = (16 * v) % W;
#pragma unroll
        for (int s = 0; s < 4; ++s) idx[s] = ((4 * lg + s) * v) % W;
        for (int t0 = 0; t0 < ntile; t0 += 16) {
            doublex4 yr[4], yi[4];
            double cur[4][4], nxt[4][4];
            int id[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                yr[q] = doublex4{0.0, 0.0, 0.0, 0.0};
                yi[q] = yr[q];
                id[q] = idx[q];
                spec_load4(img, sb, t0 + 4 * q + wave < ntile ? (t0 + 4 * q + wave) * 16 + li : H, 4 * lg, H, W, vec, cur[q], bad);
            }
            for (int x0 = 0; x0 < W; x0 += 16) {
                const bool more = x0 + 16 < W;
                if (more) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        spec_load4(img, sb, t0 + 4 * q + wave < ntile ? (t0 + 4 * q + wave) * 16 + li : H, x0 + 16 + 4 * lg, H, W, vec,
                                   nxt[q], bad);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double2 t = twW[id[s]];
                    const double c = t.x, ns = -t.y;
                    id[s] += step;
                    if (id[s] >= W) id[s] -= W;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (t0 + 4 * q + wave < ntile) {
                            yr[q] = mfma64(cur[q][s], c, yr[q]);
                            yi[q] = mfma64(cur[q][s], ns, yi[q]);
                        }
                }
                if (more) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) cur[q][e] = nxt[q][e];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int y = (t0 + 4 * q + wave) * 16 + lg + 4 * g;
                    if (y < H && li < sv) {
                        Yr[y * sv + li] = yr[q][g];
                        Yi[y * sv + li] = yi[q][g];
                    }
                }
        }
    }
    // Is the row finite?  One int in the LDS of the W table, which the rows pass is done with: __syncthreads_or would take static LDS
    // of its own on top of the dynamic block, and at H = W = 1024 that block is the whole 160 KB of a CU.  The last barrier is also
    // the one between the passes.
    int* bad_slot = reinterpret_cast<int*>(spec_lds);
    __syncthreads();
    if (threadIdx.x == 0) *bad_slot = 0;
    __syncthreads();
    if (bad) *bad_slot = 1;
    __syncthreads();
    const int anybad = *bad_slot;
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[r] = anybad;
    if (anybad) return;  // the row's bins become NaN in the third launch, whatever stands in its power plane

    // columns pass: A = e^{-2 pi i u y / H} [u][y], B = Y [y][v]:  Xr = sum c Yr + s Yi,  Xi = sum c Yi - s Yr
    const double w_v = (v0 + li == 0 || 2 * (v0 + li) == W) ? 1.0 : 2.0;
    const double hw = (double)(H * W);
    for (int t0 = 0; t0 < ntile; t0 += 16) {
        doublex4 xr[4], xi[4];
        int id[4], step[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xr[q] = doublex4{0.0, 0.0, 0.0, 0.0};
            xi[q] = xr[q];
            const int u = (t0 + 4 * q + wave) * 16 + li;
            id[q] = (u * lg) % H;
            step[q] = (4 * u) % H;
        }
        for (int y0 = 0; y0 < H; y0 += 4) {
            const int y = y0 + lg;
            double br = 0.0, bi = 0.0;
            if (y < H && li < sv) {
                br = Yr[y * sv + li];
                bi = Yi[y * sv + li];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (t0 + 4 * q + wave < ntile) {
                    const double2 t = twH[id[q]];
                    xr[q] = mfma64(t.x, br, xr[q]);
                    xr[q] = mfma64(t.y, bi, xr[q]);
                    xi[q] = mfma64(t.x, bi, xi[q]);
                    xi[q] = mfma64(-t.y, br, xi[q]);
                }
                id[q] += step[q];
                if (id[q] >= H) id[q] -= H;
            }
        }
        const int vv = v0 + li;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int u = (t0 + 4 * q + wave) * 16 + lg + 4 * g;
                if (u < H && li < sv && vv < Wh) {
                    const double m2 = __fma_rn(xr[q][g], xr[q][g], __dmul_rn(xi[q][g], xi[q][g]));
                    power[(r * H + u) * Wh + vv] = __dmul_rn(__ddiv_rn(m2, hw), w_v);
                }
            }
    }
}

__global__ __launch_bounds__(64 * SPEC_BIN_WAVES) void spectrum_bin_kernel(const double* __restrict__ power, const int32_t* __restrict__ bins,
                                                                           const int32_t* __restrict__ flags, double* __restrict__ out, int nb,
                                                                           int H, int Wh) {
    __shared__ double red[SPEC_BIN_WAVES][64];
    __shared__ __attribute__((aligned(16))) int32_t sbin[SPEC_BIN_WAVES][SPEC_BIN_CHUNK];
    __shared__ __attribute__((aligned(16))) double spow[SPEC_BIN_WAVES][SPEC_BIN_CHUNK];
    const long long r = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long k = (long long)blockIdx.x * 64 + lane;
    if (flags[r]) {
        if (wave == 0 && k < nb) out[r * nb + k] = __longlong_as_double((long long)QNAN64_BITS);
        return;
    }
    const int kk = k < nb ? (int)k : -2;  // a lane past nb owns no bin; -1 marks a staged slot past the plane's end
    double acc = 0.0;
    // The plane's H * Wh points in index order, SPEC_BIN_WAVES * SPEC_BIN_CHUNK at a time through LDS: staged by the whole block (the
    // next piece is requested before this one is scanned), then wave w scans the w-th SPEC_BIN_CHUNK points of the piece.
    constexpr int PIECE = SPEC_BIN_WAVES * SPEC_BIN_CHUNK, PER = PIECE / (64 * SPEC_BIN_WAVES);
    const long long n = (long long)H * Wh;
    const double* __restrict__ pr = power + r * n;
    int32_t* sb = &sbin[0][0];
    double* sp = &spow[0][0];
    int32_t nb_[PER];
    double np_[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const long long p = threadIdx.x + (long long)e * blockDim.x;
        nb_[e] = p < n ? bins[p] : -1;
        np_[e] = p < n ? pr[p] : 0.0;
    }
    for (long long p0 = 0; p0 < n; p0 += PIECE) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            sb[threadIdx.x + e * blockDim.x] = nb_[e];
            sp[threadIdx.x + e * blockDim.x] = np_[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const long long p = p0 + PIECE + threadIdx.x + (long long)e * blockDim.x;
            nb_[e] = p < n ? bins[p] : -1;
            np_[e] = p < n ? pr[p] : 0.0;
        }
        if (p0 + (long long)wave * SPEC_BIN_CHUNK >= n) continue;  // nothing of this piece is left for the wave
        const int4* b4 = reinterpret_cast<const int4*>(sbin[wave]);
        const double2* p2 = reinterpret_cast<const double2*>(spow[wave]);
#pragma unroll 4
        for (int j = 0; j < SPEC_BIN_CHUNK / 4; ++j) {
            const int4 b = b4[j];
            const double2 pa = p2[2 * j], pb = p2[2 * j + 1];
            acc = b.x == kk ? __dadd_rn(acc, pa.x) : acc;
            acc = b.y == kk ? __dadd_rn(acc, pa.y) : acc;
            acc = b.z == kk ? __dadd_rn(acc, pb.x) : acc;
            acc = b.w == kk ? __dadd_rn(acc, pb.y) : acc;
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && k < nb) {
        double s = red[0][lane];
#pragma unroll
        for (int w = 1; w < SPEC_BIN_WAVES; ++w) s = __dadd_rn(s, red[w][lane]);
        out[r * nb + k] = s;
    }
}

}  // namespace

extern "C" int64_t idiff_radial_power_spectrum_ws_bytes(int R, int H, int W) {
    if (R <= 0 || R > 65535 || H <= 0 || H > SPEC_MAX_N || W <= 0 || W > SPEC_MAX_N) return 0;
    return spec_ws_layout(R, H, W).total;
}

extern "C" int idiff_radial_power_spectrum(const float* x, const float* sub, int sub_rep, const int32_t* bins, int nb, double* out, void* ws,
                                           int R, int H, int W, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && bins && out && ws && R > 0 && R <= 65535, "radial_power_spectrum: bad args");
    IDIFF_CHECK_ARG(H >= 1 && H <= SPEC_MAX_N && W >= 1 && W <= SPEC_MAX_N, "radial_power_spectrum: H = %d, W = %d are outside [1, %d]", H, W,
                    SPEC_MAX_N);
    IDIFF_CHECK_ARG(nb >= 1, "radial_power_spectrum: nb = %d is not positive", nb);
    IDIFF_CHECK_ARG(!sub || (sub_rep >= 1 && R % sub_rep == 0), "radial_power_spectrum: sub_rep = %d does not divide R = %d", sub_rep, R);
    IDIFF_CHECK_ARG((((uintptr_t)x | (uintptr_t)sub | (uintptr_t)bins) & 3) == 0 && (((uintptr_t)out | (uintptr_t)ws) & 7) == 0,
                    "radial_power_spectrum: x, sub and bins must be 4-byte aligned, out and ws 8-byte aligned");
    const spec_ws l = spec_ws_layout(R, H, W);
    char* base = static_cast<char*>(ws);
    double2* tab = reinterpret_cast<double2*>(base + l.tab);
    int32_t* flags = reinterpret_cast<int32_t*>(base + l.flags);
    double* power = reinterpret_cast<double*>(base + l.power);
    hipStream_t st = (hipStream_t)stream;
    const int sv = spec_strip(H), Wh = W / 2 + 1;
    const int vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)sub) & 15) == 0;
    const size_t lds = 16ull * (W + H) + 16ull * H * sv;
    static idiff_dyn_lds_cache lds_cache;
    if (int e = idiff_dyn_lds(lds_cache, spectrum_dft_kernel, lds, "radial_power_spectrum")) return e;
    hipLaunchKernelGGL(spectrum_twiddle_kernel, dim3((unsigned)((W + H + 255) / 256)), dim3(256), 0, st, tab, W, H);
    IDIFF_CHECK_LAUNCH("radial_power_spectrum_twiddle");
    hipLaunchKernelGGL(spectrum_dft_kernel, dim3((unsigned)((Wh + sv - 1) / sv), (unsigned)R), dim3(256), lds, st, x, sub, sub ? sub_rep : 1,
                       (const double2*)tab, flags, power, H, W, vec);
    IDIFF_CHECK_LAUNCH("radial_power_spectrum_dft");
    hipLaunchKernelGGL(spectrum_bin_kernel, dim3((unsigned)((nb + 63) / 64), (unsigned)R), dim3(64 * SPEC_BIN_WAVES), 0, st,
                       (const double*)power, bins, (const int32_t*)flags, out, nb, H, Wh);
    IDIFF_CHECK_LAUNCH("radial_power_spectrum_bin");
    return IDIFF_OK;
}
