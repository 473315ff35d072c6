// Principal modes of a posterior ensemble (include/idiff.h: idiff_ensemble_modes, idiff_ensemble_modes_pair, idiff_ensemble_project;
// DESIGN.md §3).  idiff_ensemble_distances' matrix of squared distances is an exact linear image of the members' centred Gram matrix, so
// the spectrum needs no further pass over the images: one block per image centres the matrix in LDS, diagonalises the S x S member block
// by a parallel cyclic two-sided Jacobi iteration and writes the sorted spectrum, the eigenvectors, the coefficients of the unit-norm mode
// images and the coordinates of the target.  A second, streaming kernel applies any [K][S] coefficients to the centred members.
//
// Modes kernel: fp64 throughout, G and V in LDS at a pitch of 65 doubles (a column walk then steps 130 dwords = 2 banks: conflict-free
// for the 32 lanes of a ds_read_b64 group), no atomics, block barriers only, every trip count bounded by (32 sweeps, Sp - 1 rounds).
// Project kernel: 256 threads, one float4 per lane and member, grid-stride over at most 64 chunks per image; the K*S coefficients sit in
// LDS; members stay in registers for S <= 16 and are read a second time above that; fp64 per pixel, members in index order.
#include "common.h"

#include <initializer_list>

namespace {

constexpr int MODES_MAX_S = 64;
constexpr int MODES_PITCH = 65;       // doubles per row of G and of V
constexpr int MODES_MAX_SWEEPS = 32;  // the cap that bounds the kernel's run time whatever the matrix
constexpr int MODES_MAX_PAIRS = MODES_MAX_S / 2;
constexpr size_t MODES_LDS_BYTES = 2 * (size_t)MODES_MAX_S * MODES_PITCH * sizeof(double);
constexpr int PROJ_MAX_K = 8;
constexpr int PROJ_REG = 16;    // members kept in registers (= ENS_REG of ensemble_stats)
constexpr int PROJ_PARTS = 64;  // chunks per image at most
constexpr unsigned QNAN_BITS = 0x7fc00000u;

// The round-robin ("circle") schedule.  Sp = S rounded up to even; round r of Sp - 1 holds Sp / 2 disjoint pairs: pair 0 is
// (r, Sp - 1), pair i >= 1 is ((r + i) mod (Sp - 1), (r - i) mod (Sp - 1)).  Over the rounds every pair of 0 .. Sp - 1 occurs once.
// Returns false for a pair that touches the padding index (S odd: index S), else p < q.
__host__ __device__ inline bool modes_pair(int S, int round, int i, int& p, int& q) {
    const int Sp = S + (S & 1), n = Sp - 1;
    const int a = i == 0 ? round : (round + i) % n;
    const int b = i == 0 ? Sp - 1 : (round - i + n) % n;
    if (a >= S || b >= S) return false;
    p = a < b ? a : b;
    q = a < b ? b : a;
    return true;
}

__global__ __launch_bounds__(256) void ensemble_modes_kernel(const double* __restrict__ d2, int S, int M, double rel_floor,
                                                             double* __restrict__ lam, double* __restrict__ vec, double* __restrict__ coef,
                                                             double* __restrict__ tcoord, double* __restrict__ tnorm2,
                                                             int32_t* __restrict__ info) {
    extern __shared__ double modes_lds[];
    constexpr int P = MODES_PITCH;
    double* G = modes_lds;
    double* V = modes_lds + MODES_MAX_S * P;  // holds the member block of d2 until G is formed
    __shared__ double sa[MODES_MAX_S + 1], sh[MODES_MAX_S + 1], sdt[MODES_MAX_S], sg[MODES_MAX_S], slam[MODES_MAX_S], ssgn[MODES_MAX_S];
    __shared__ double rc[MODES_MAX_PAIRS], rs[MODES_MAX_PAIRS];
    __shared__ int rp[MODES_MAX_PAIRS], rq[MODES_MAX_PAIRS], sord[MODES_MAX_S];
    const int t = threadIdx.x;
    const long long b = blockIdx.x;
    const double* D = d2 + b * M * M;
    double* lam_b = lam + b * S;
    double* vec_b = vec + b * S * S;
    double* coef_b = coef + b * S * S;
    double* tc_b = tcoord + b * S;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    // the upper triangle only: the diagonal counts as 0, the lower half is never read
    int bad = 0;
    for (int idx = t; idx < M * M; idx += blockDim.x) {
        const int i = idx / M, j = idx - i * M;
        if (i < j) {
            const double v = D[idx];
            if (!(v >= 0.0 && v < __builtin_inf())) bad = 1;
            if (j < S) {
                V[i * P + j] = v;
                V[j * P + i] = v;
            } else {
                sdt[i] = v;
            }
        } else if (i == j && i < S) {
            V[i * P + i] = 0.0;
        }
    }
    if (__syncthreads_or(bad)) {
        for (int idx = t; idx < S * S; idx += blockDim.x) {
            vec_b[idx] = 0.0;
            coef_b[idx] = 0.0;
        }
        if (t < S) {
            lam_b[t] = qnan;
            tc_b[t] = qnan;
        }
        if (t == 0) {
            tnorm2[b] = qnan;
            info[b * 2] = -1;
            info[b * 2 + 1] = 0;
        }
        return;
    }

    // centring about the members' centroid: a_i, abar, h_i = |r_i - c|^2, G_ij = <r_i - c, r_j - c>; every sum in index order
    const double dS = (double)S;
    if (t < M) {
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc = __dadd_rn(acc, t < S ? V[t * P + s] : sdt[s]);
        sa[t] = __ddiv_rn(acc, dS);
    }
    __syncthreads();
    double abar = 0.0;
    for (int s = 0; s < S; ++s) abar = __dadd_rn(abar, sa[s]);
    abar = __ddiv_rn(abar, dS);
    if (t < M) sh[t] = __dsub_rn(sa[t], __dmul_rn(0.5, abar));
    __syncthreads();
    for (int idx = t; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx - i * S;
        G[i * P + j] = __dmul_rn(0.5, __dsub_rn(__dadd_rn(sh[i], sh[j]), V[i * P + j]));
    }
    if (M > S && t < S) sg[t] = __dmul_rn(0.5, __dsub_rn(__dadd_rn(sh[S], sh[t]), sdt[t]));
    __syncthreads();
    for (int idx = t; idx < S * S; idx += blockDim.x) {
        const int i = idx / S, j = idx - i * S;
        V[i * P + j] = i == j ? 1.0 : 0.0;
    }
    double tr0 = 0.0;
    for (int i = 0; i < S; ++i) tr0 = __dadd_rn(tr0, G[i * P + i]);
    const double thresh = __dmul_rn(0x1p-53, tr0);
    __syncthreads();

    // parallel cyclic two-sided Jacobi; a degenerate image (tr0 == 0: S = 1, no valid pixel, all members equal) keeps G = 0, V = I
    int sweeps = 0;
    if (tr0 > 0.0) {
        sweeps = -1;
        const int Sp = S + (S & 1), np = Sp / 2, nr = Sp - 1;
        for (int sw = 1; sw <= MODES_MAX_SWEEPS; ++sw) {
            int rotated = 0;
            for (int r = 0; r < nr; ++r) {
                // (a) the rotations of this round's pairs, from the current matrix (Rutishauser's formulas)
                if (t < np) {
                    int p = -1, q = 0;
                    if (modes_pair(S, r, t, p, q)) {
                        const double gpq = G[p * P + q];
                        if (fabs(gpq) > thresh) {
                            const double th = __ddiv_rn(__dsub_rn(G[q * P + q], G[p * P + p]), __dmul_rn(2.0, gpq));
                            const double tt = __ddiv_rn(th >= 0.0 ? 1.0 : -1.0, __dadd_rn(fabs(th), hypot(1.0, th)));
                            const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(tt, tt), 1.0)));
                            rc[t] = c;
                            rs[t] = __dmul_rn(tt, c);
                            rotated = 1;
                        } else {
                            p = -1;
                        }
                    } else {
                        p = -1;
                    }
                    rp[t] = p;
                    rq[t] = q;
                }
                __syncthreads();
                // (b) columns p, q of G and of V: item = (pair, matrix, row), the row fastest
                for (int it = t; it < np * 2 * S; it += blockDim.x) {
                    const int k = it % S, w = (it / S) & 1, pr = it / (2 * S);
                    const int p = rp[pr];
                    if (p < 0) continue;
                    const int q = rq[pr];
                    const double c = rc[pr], s = rs[pr];
                    double* A = w ? V : G;
                    const double x = A[k * P + p], y = A[k * P + q];
                    A[k * P + p] = __dsub_rn(__dmul_rn(c, x), __dmul_rn(s, y));
                    A[k * P + q] = __dadd_rn(__dmul_rn(s, x), __dmul_rn(c, y));
                }
                __syncthreads();
                // (c) rows p, q of G: item = (pair, column), the column fastest
                for (int it = t; it < np * S; it += blockDim.x) {
                    const int k = it % S, pr = it / S;
                    const int p = rp[pr];
                    if (p < 0) continue;
                    const int q = rq[pr];
                    const double c = rc[pr], s = rs[pr];
                    const double x = G[p * P + k], y = G[q * P + k];
                    G[p * P + k] = __dsub_rn(__dmul_rn(c, x), __dmul_rn(s, y));
                    G[q * P + k] = __dadd_rn(__dmul_rn(s, x), __dmul_rn(c, y));
                }
                __syncthreads();
                // (d) the rotated pairs are annihilated exactly
                if (t < np && rp[t] >= 0) {
                    G[rp[t] * P + rq[t]] = 0.0;
                    G[rq[t] * P + rp[t]] = 0.0;
                }
                __syncthreads();
            }
            if (!__syncthreads_or(rotated)) {
                sweeps = sw;
                break;
            }
        }
    }

    // descending order by a counting rank, ties by the original column; then the sign of each eigenvector
    if (t < S) {
        slam[t] = G[t * P + t];
        sord[t] = t;  // every slot holds a member even if an overflowed (NaN) spectrum leaves a rank untaken
    }
    __syncthreads();
    if (t < S) {
        const double lt = slam[t];
        int r = 0;
        for (int i = 0; i < S; ++i) {
            const double li = slam[i];
            r += (li > lt || (li == lt && i < t)) ? 1 : 0;
        }
        sord[r < S ? r : S - 1] = t;
    }
    __syncthreads();
    bool live = false;
    double lk = 0.0;
    if (t < S) {
        const int j = sord[t];
        double big = -1.0, sgn = 1.0;
        for (int s = 0; s < S; ++s) {
            const double v = V[s * P + j];
            if (fabs(v) > big) {
                big = fabs(v);
                sgn = v < 0.0 ? -1.0 : 1.0;
            }
        }
        ssgn[t] = sgn;
        const double l0 = slam[sord[0]];
        lk = slam[j];
        live = l0 > 0.0 && lk > __dmul_rn(rel_floor, l0);
    }
    const int rank = __syncthreads_count(live ? 1 : 0);
    for (int idx = t; idx < S * S; idx += blockDim.x) {
        const int k = idx / S, s = idx - k * S;
        const int j = sord[k];
        const double l0 = slam[sord[0]], l = slam[j];
        const double v = __dmul_rn(ssgn[k], V[s * P + j]);
        vec_b[idx] = v;
        coef_b[idx] = (l0 > 0.0 && l > __dmul_rn(rel_floor, l0)) ? __ddiv_rn(v, __dsqrt_rn(l)) : 0.0;
    }
    if (t < S) {
        lam_b[t] = lk;
        double tk = 0.0;
        if (M > S && live) {
            const int j = sord[t];
            double acc = 0.0;
            for (int s = 0; s < S; ++s) acc = __fma_rn(__dmul_rn(ssgn[t], V[s * P + j]), sg[s], acc);
            tk = __ddiv_rn(acc, __dsqrt_rn(lk));
        }
        tc_b[t] = tk;
    }
    if (t == 0) {
        tnorm2[b] = M > S ? sh[S] : 0.0;
        info[b * 2] = rank;
        info[b * 2 + 1] = sweeps;
    }
}

// out[b][k][pixel] = sum_s coef[b][k][s] (x[b][s][pixel] - c), c the pixel's member mean; fp64, members in index order.
template <bool REG>
__global__ __launch_bounds__(256) void ensemble_project_kernel(const float* __restrict__ x, const double* __restrict__ coef, long long cstride,
                                                               float* __restrict__ out, int S, int K, long long Q) {
    __shared__ double cf[PROJ_MAX_K * MODES_MAX_S];
    const long long b = blockIdx.y;
    for (int i = threadIdx.x; i < K * S; i += blockDim.x) cf[i] = coef[b * cstride + i];
    __syncthreads();
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + b * S * Q;
    floatx4* o = reinterpret_cast<floatx4*>(out) + b * K * Q;
    const double dS = (double)S;
    const float qn = __uint_as_float(QNAN_BITS);
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        floatx4 val[REG ? PROJ_REG : 1];
        double c[4];
        bool ok[4];
        {
            const floatx4 x0 = xs[v];
            if (REG) val[0] = x0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = (double)x0[e];
                ok[e] = fabsf(x0[e]) < __builtin_inff();
            }
        }
        if (REG) {
#pragma unroll
            for (int s = 1; s < PROJ_REG; ++s)
                if (s < S) val[s] = xs[(long long)s * Q + v];
#pragma unroll
            for (int s = 1; s < PROJ_REG; ++s)
                if (s < S)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        c[e] = __dadd_rn(c[e], (double)val[s][e]);
                        ok[e] &= fabsf(val[s][e]) < __builtin_inff();
                    }
        } else {
            for (int s = 1; s < S; ++s) {
                const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    c[e] = __dadd_rn(c[e], (double)xv[e]);
                    ok[e] &= fabsf(xv[e]) < __builtin_inff();
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = __ddiv_rn(c[e], dS);
        if (REG) {
            // one plane at a time: the differences are formed again per plane (same operands, same bits), which keeps the live
            // registers at the members and one plane's four sums
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < PROJ_REG; ++s)
                    if (s < S) {
                        const double w = cf[k * S + s];
#pragma unroll
                        for (int e = 0; e < 4; ++e) a[e] = __fma_rn(w, __dsub_rn((double)val[s][e], c[e]), a[e]);
                    }
                floatx4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = ok[e] ? (float)a[e] : qn;
                o[(long long)k * Q + v] = r;
            }
            continue;
        }
        double acc[PROJ_MAX_K][4];
#pragma unroll
        for (int k = 0; k < PROJ_MAX_K; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;
        {
            for (int s = 0; s < S; ++s) {
                const floatx4 xv = xs[(long long)s * Q + v];
                double d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = __dsub_rn((double)xv[e], c[e]);
#pragma unroll
                for (int k = 0; k < PROJ_MAX_K; ++k)
                    if (k < K) {
                        const double w = cf[k * S + s];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[k][e] = __fma_rn(w, d[e], acc[k][e]);
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < PROJ_MAX_K; ++k)
            if (k < K) {
                floatx4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = ok[e] ? (float)acc[k][e] : qn;
                o[(long long)k * Q + v] = r;
            }
    }
}

inline bool aligned_to(std::initializer_list<const void*> ps, uintptr_t a) {
    uintptr_t bits = 0;
    for (const void* p : ps) bits |= (uintptr_t)p;
    return bits % a == 0;
}
// [p, p + bytes) and [q, q + qbytes) share no byte
inline bool apart(const void* p, unsigned long long bytes, const void* q, unsigned long long qbytes) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p0 + bytes <= q0 || q0 + qbytes <= p0;
}

}  // namespace

extern "C" int idiff_ensemble_modes_pair(int S, int round, int i, int* p, int* q) {
    IDIFF_CHECK_ARG(p && q && S >= 1 && S <= MODES_MAX_S, "ensemble_modes_pair: S = %d is outside [1, %d], or a null pointer", S, MODES_MAX_S);
    const int Sp = S + (S & 1);
    IDIFF_CHECK_ARG(round >= 0 && round < Sp - 1 && i >= 0 && i < Sp / 2, "ensemble_modes_pair: round %d / pair %d is outside [0, %d) x [0, %d)",
                    round, i, Sp - 1, Sp / 2);
    int a = -1, b = -1;
    const bool real = modes_pair(S, round, i, a, b);
    *p = real ? a : -1;
    *q = real ? b : -1;
    return real ? 1 : 0;
}

extern "C" int idiff_ensemble_modes(const double* d2, int B, int S, int has_target, double rel_floor, double* lam, double* vec, double* coef,
                                    double* tcoord, double* tnorm2, int32_t* info, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(d2 && lam && vec && coef && tcoord && tnorm2 && info && B > 0 && B <= 65535, "ensemble_modes: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= MODES_MAX_S, "ensemble_modes: S = %d is outside [1, %d]", S, MODES_MAX_S);
    IDIFF_CHECK_ARG(rel_floor > 0.0 && rel_floor < 1.0, "ensemble_modes: rel_floor = %g is outside (0, 1)", rel_floor);
    IDIFF_CHECK_ARG(aligned_to({d2, lam, vec, coef, tcoord, tnorm2, info}, 8), "ensemble_modes: every buffer must be 8-byte aligned");
    const int M = S + (has_target ? 1 : 0);
    const unsigned long long ub = (unsigned long long)B;
    const void* bufs[] = {d2, lam, vec, coef, tcoord, tnorm2, info};
    const unsigned long long bytes[] = {8ull * ub * M * M, 8ull * ub * S, 8ull * ub * S * S, 8ull * ub * S * S, 8ull * ub * S, 8ull * ub, 8ull * ub};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            IDIFF_CHECK_ARG(apart(bufs[i], bytes[i], bufs[j], bytes[j]), "ensemble_modes: d2, lam, vec, coef, tcoord, tnorm2 and info must not overlap");
    static idiff_dyn_lds_cache lds_cache;
    if (const int rc = idiff_dyn_lds(lds_cache, ensemble_modes_kernel, MODES_LDS_BYTES, "ensemble_modes")) return rc;
    hipLaunchKernelGGL(ensemble_modes_kernel, dim3((unsigned)B), dim3(256), MODES_LDS_BYTES, (hipStream_t)stream, d2, S, M, rel_floor, lam, vec, coef,
                       tcoord, tnorm2, info);
    IDIFF_CHECK_LAUNCH("ensemble_modes");
    return IDIFF_OK;
}

extern "C" int idiff_ensemble_project(const float* x, const double* coef, int64_t coef_image_stride, float* out, int B, int S, int K, int64_t n_s,
                                      idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && coef && out && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL, "ensemble_project: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= MODES_MAX_S, "ensemble_project: S = %d is outside [1, %d]", S, MODES_MAX_S);
    IDIFF_CHECK_ARG(K >= 1 && K <= PROJ_MAX_K, "ensemble_project: K = %d is outside [1, %d]", K, PROJ_MAX_K);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_project: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(coef_image_stride >= (int64_t)K * S, "ensemble_project: coef_image_stride = %lld is below K * S = %d",
                    (long long)coef_image_stride, K * S);
    IDIFF_CHECK_ARG(aligned_to({x, out}, 16) && aligned_to({coef}, 8), "ensemble_project: x and out must be 16-byte aligned, coef 8-byte aligned");
    const unsigned long long xb = 4ull * B * S * n_s, ob = 4ull * B * K * n_s,
                             cb = 8ull * ((unsigned long long)(B - 1) * coef_image_stride + (unsigned long long)K * S);
    IDIFF_CHECK_ARG(apart(out, ob, x, xb) && apart(out, ob, coef, cb), "ensemble_project: out must not overlap x or coef");
    const long long Q = n_s / 4;
    long long gx = (Q + 255) / 256;
    if (gx > PROJ_PARTS) gx = PROJ_PARTS;
    const dim3 grid((unsigned)gx, (unsigned)B);
    if (S <= PROJ_REG)
        hipLaunchKernelGGL(ensemble_project_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, coef, (long long)coef_image_stride, out, S, K, Q);
    else
        hipLaunchKernelGGL(ensemble_project_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, coef, (long long)coef_image_stride, out, S, K, Q);
    IDIFF_CHECK_LAUNCH("ensemble_project");
    return IDIFF_OK;
}
