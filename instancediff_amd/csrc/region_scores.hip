// Region-wise ensemble scores over an integer label map (include/idiff.h: idiff_region_scores, idiff_band_labels).
// The per-pixel record is idiff_ensemble_scores' (sde.hip), operation for operation, plus the signed mean error m.  Like sde.o the
// object is built with -ffp-contract=off (Makefile): the rounding intrinsics are plain operators to the compiler.
//
// Launch 1, 64 x B blocks of 256 threads (region_scores_kernel).  Thread (p, tid) takes float4 v = p*256 + tid + i*16384 in sweep i and
// its four labels as one 32-bit load; every lane runs all ceil(Q / 16384) sweeps, a lane past the end of the image with nothing to add,
// so every shuffle below runs with 64 active lanes.  Per sweep: the histogram bins of the four pixels (integer LDS adds, the label
// compared against L first); the wave's set of labels < L carried by a valid pixel as a 64-bit word (an OR over the xor tree, read
// back through readfirstlane: wave-uniform); then for each label of the set and each of the four quantities the lane's fp64 sum of its
// matching elements in element order from +0.0, the fixed xor tree (offsets 32 .. 1), and lane 0 adds the wave's sum to the wave's LDS
// slot [wave][label][quantity] -- sweep order.  At the end the four waves' slots are added in wave order: one fp64 partial per block,
// label and quantity.  There is no per-thread per-label accumulator: 64 labels x 4 quantities of fp64 per lane would be 512 VGPRs or an
// LDS array of 512 KiB per block, and a data-dependent register index is scratch; the wave-level set costs one tree per label present,
// 1 - 3 on a spatially coherent map.
// Launch 2, one block per image (region_scores_final_kernel): adds the 64 partials of every (label, quantity) and of every bin in
// index order.  Integer LDS adds are the only atomics.
#include "common.h"

#include <math.h>
#include <stdlib.h>

namespace {

constexpr int RS_PARTS = 64;  // partial blocks per image (= SCORE_PARTS)
constexpr int RS_MAX_S = 64;
constexpr int RS_MAX_L = 64;
constexpr int RS_REG = 16;    // the register form's largest S (= SCORE_REG)
constexpr int RS_CH = 4;      // candidates per chunk of the second-read form (= SCORE_CH)
constexpr int RS_NQ = 4;      // crps, e, v, m
constexpr int BAND_MAX_E = 63;

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

// The four pixels of a float4: the fp32 quantities, the histogram bin (k, or S + 1 where invalid) and validity.
struct PixRec {
    floatx4 q[RS_NQ];
    int bin[4];
    bool ok[4];
};

// The end of a pixel, as score_pixel in sde.hip: two correctly rounded quotients and one subtraction; k <= S by construction.
__device__ __forceinline__ void finish_pixel(PixRec& r, int e, float a, float g, float ss, float m, int k, bool bad, int S) {
    r.q[0][e] = __fsub_rn(__fdiv_rn(a, (float)S), __fdiv_rn(g, (float)(S * S)));
    r.q[1][e] = __fmul_rn(m, m);
    r.q[2][e] = S > 1 ? __fdiv_rn(ss, (float)(S - 1)) : 0.f;
    r.q[3][e] = m;
    r.bin[e] = bad ? S + 1 : k;
    r.ok[e] = !bad;
}

// Register form, S <= 16: ensemble_scores_reg_kernel's pixel loop (one compare per unordered pair).
template <int S>
__device__ __forceinline__ void pixels_reg(const floatx4* __restrict__ xs, floatx4 y, long long Q, long long v, PixRec& r) {
    floatx4 d[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[s][e] = __fsub_rn(xv[e], y[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float a = 0.f, g = 0.f, sd = 0.f, ss = 0.f;
        int k = 0;
        bool bad = false;
        int rank[S];
#pragma unroll
        for (int s = 0; s < S; ++s) rank[s] = S - 1 - s;
#pragma unroll
        for (int s = 1; s < S; ++s)
#pragma unroll
            for (int j = 0; j < s; ++j) {
                const int le = d[j][e] <= d[s][e] ? 1 : 0;
                rank[s] += le;
                rank[j] -= le;
            }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float ds = d[s][e];
            const float term = __fmul_rn((float)(2 * rank[s] - S + 1), ds);
            bad |= ds != ds;
            k += ds < 0.f ? 1 : 0;
            a = s == 0 ? fabsf(ds) : __fadd_rn(a, fabsf(ds));
            g = s == 0 ? term : __fadd_rn(g, term);
            sd = s == 0 ? ds : __fadd_rn(sd, ds);
        }
        const float m = __fdiv_rn(sd, (float)S);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float t = __fsub_rn(d[s][e], m);
            ss = s == 0 ? __fmul_rn(t, t) : __fadd_rn(ss, __fmul_rn(t, t));
        }
        finish_pixel(r, e, a, g, ss, m, k, bad, S);
    }
}

// Second-read form, any S: ensemble_scores_reread_kernel's pixel loop; the same operations in the same order as the register form.
__device__ __forceinline__ void pixels_reread(const floatx4* __restrict__ xs, floatx4 y, long long Q, long long v, int S, PixRec& r) {
    floatx4 a = {0.f, 0.f, 0.f, 0.f}, g = a, sd = a, ss = a, mv;
    int k[4] = {0, 0, 0, 0};
    bool bad[4] = {false, false, false, false};
    for (int s = 0; s < S; ++s) {
        const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ds = __fsub_rn(xv[e], y[e]);
            bad[e] |= ds != ds;
            k[e] += ds < 0.f ? 1 : 0;
            a[e] = s == 0 ? fabsf(ds) : __fadd_rn(a[e], fabsf(ds));
            sd[e] = s == 0 ? ds : __fadd_rn(sd[e], ds);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) mv[e] = __fdiv_rn(sd[e], (float)S);
    for (int s0 = 0; s0 < S; s0 += RS_CH) {
        floatx4 cand[RS_CH];
        int rank[RS_CH][4];
#pragma unroll
        for (int c = 0; c < RS_CH; ++c) {
            const int s = s0 + c < S ? s0 + c : S - 1;  // past the end: a copy of the last member, added to nothing
            const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cand[c][e] = __fsub_rn(xv[e], y[e]);
                rank[c][e] = 0;
            }
        }
        for (int j = 0; j < s0; ++j) {
            const floatx4 xj = xs[(long long)j * Q + v];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dj = __fsub_rn(xj[e], y[e]);
#pragma unroll
                for (int c = 0; c < RS_CH; ++c) rank[c][e] += dj <= cand[c][e] ? 1 : 0;
            }
        }
#pragma unroll
        for (int jj = 0; jj < RS_CH; ++jj)
            if (s0 + jj < S) {
#pragma unroll
                for (int c = 0; c < RS_CH; ++c) {
                    if (c == jj) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) rank[c][e] += (jj < c ? cand[jj][e] <= cand[c][e] : cand[jj][e] < cand[c][e]) ? 1 : 0;
                }
            }
        for (int j = s0 + RS_CH; j < S; ++j) {
            const floatx4 xj = xs[(long long)j * Q + v];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dj = __fsub_rn(xj[e], y[e]);
#pragma unroll
                for (int c = 0; c < RS_CH; ++c) rank[c][e] += dj < cand[c][e] ? 1 : 0;
            }
        }
#pragma unroll
        for (int c = 0; c < RS_CH; ++c)
            if (s0 + c < S) {
                const bool first = s0 + c == 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float term = __fmul_rn((float)(2 * rank[c][e] - S + 1), cand[c][e]);
                    const float t = __fsub_rn(cand[c][e], mv[e]);
                    g[e] = first ? term : __fadd_rn(g[e], term);
                    ss[e] = first ? __fmul_rn(t, t) : __fadd_rn(ss[e], __fmul_rn(t, t));
                }
            }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) finish_pixel(r, e, a[e], g[e], ss[e], mv[e], k[e], bad[e], S);
}

// ST > 0: the register form of S = ST; ST = 0: the second-read form of S = s_rt.  Every lane of every wave reaches every shuffle.
template <int ST>
__global__ __launch_bounds__(256) void region_scores_kernel(const float* __restrict__ x, const float* __restrict__ tgt,
                                                            const uint8_t* __restrict__ labels, long long labels_bstride, int L,
                                                            double* __restrict__ part_sums, int32_t* __restrict__ part_hist,
                                                            int32_t* __restrict__ part_out, int s_rt, long long Q) {
    __shared__ int hist[RS_MAX_L * (RS_MAX_S + 2)];
    __shared__ double slot[4][RS_MAX_L * RS_NQ];
    __shared__ int out_lds;
    const int S = ST ? ST : s_rt;
    const int nb = L * (S + 2), nq = L * RS_NQ;
    for (int i = threadIdx.x; i < nb; i += 256) hist[i] = 0;
    for (int i = threadIdx.x; i < 4 * RS_MAX_L * RS_NQ; i += 256) (&slot[0][0])[i] = 0.0;
    if (threadIdx.x == 0) out_lds = 0;
    __syncthreads();
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + (long long)blockIdx.y * Q;
    const uint32_t* l4 = reinterpret_cast<const uint32_t*>(labels + (long long)blockIdx.y * labels_bstride);
    const int lane = threadIdx.x & 63;
    double* myslot = slot[threadIdx.x >> 6];
    const long long stride = (long long)RS_PARTS * 256;
    const long long sweeps = (Q + stride - 1) / stride;  // the same for every lane of the grid
    int outside = 0;
    for (long long i = 0; i < sweeps; ++i) {
        const long long v = i * stride + (long long)blockIdx.x * 256 + threadIdx.x;
        int sel[4] = {-1, -1, -1, -1};  // the label of a valid pixel inside [0, L), else -1
        PixRec r;
#pragma unroll
        for (int q = 0; q < RS_NQ; ++q) r.q[q] = floatx4{0.f, 0.f, 0.f, 0.f};
        unsigned long long mine = 0;
        if (v < Q) {
            const floatx4 y = t4[v];
            const uint32_t lw = l4[v];
            if constexpr (ST > 0)
                pixels_reg<ST>(xs, y, Q, v, r);
            else
                pixels_reread(xs, y, Q, v, S, r);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lab = (int)((lw >> (8 * e)) & 0xffu);
                if (lab < L) {  // checked before it becomes an index
                    atomicAdd(&hist[lab * (S + 2) + r.bin[e]], 1);
                    if (r.ok[e]) {
                        sel[e] = lab;
                        mine |= 1ull << lab;
                    }
                } else {
                    ++outside;
                }
            }
        }
        // all 64 lanes from here on
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine |= __shfl_xor(mine, o, 64);
        const unsigned set_lo = __builtin_amdgcn_readfirstlane((unsigned)mine);  // readfirstlane returns int: through unsigned first
        const unsigned set_hi = __builtin_amdgcn_readfirstlane((unsigned)(mine >> 32));
        unsigned long long present = ((unsigned long long)set_hi << 32) | set_lo;
        while (present) {  // wave-uniform
            const int l = __builtin_ctzll(present);
            present &= present - 1;
#pragma unroll
            for (int q = 0; q < RS_NQ; ++q) {
                double c = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (sel[e] == l) c = __dadd_rn(c, (double)r.q[q][e]);
                c = wave_sum_f64(c);
                if (lane == 0) myslot[l * RS_NQ + q] = __dadd_rn(myslot[l * RS_NQ + q], c);
            }
        }
    }
    if (outside) atomicAdd(&out_lds, outside);
    __syncthreads();  // every LDS add and every slot of the block has landed
    const long long blk = (long long)blockIdx.y * RS_PARTS + blockIdx.x;
    if ((int)threadIdx.x < nq) {
        const int t = threadIdx.x;
        part_sums[blk * nq + t] = __dadd_rn(__dadd_rn(__dadd_rn(slot[0][t], slot[1][t]), slot[2][t]), slot[3][t]);
    }
    for (int i = threadIdx.x; i < nb; i += 256) part_hist[blk * nb + i] = hist[i];
    if (threadIdx.x == 0) part_out[blk] = out_lds;
}

// One block per image: the 64 partials of a (label, quantity) in index order by one thread (coalesced across the threads); integer bins
// in any order give the same count.
__global__ __launch_bounds__(256) void region_scores_final_kernel(const double* __restrict__ part_sums, const int32_t* __restrict__ part_hist,
                                                                  const int32_t* __restrict__ part_out, double* __restrict__ sums,
                                                                  int32_t* __restrict__ counts, int32_t* __restrict__ outside, int L, int S) {
    const long long b = blockIdx.x;
    const int nb = L * (S + 2), nq = L * RS_NQ;
    if ((int)threadIdx.x < nq) {
        const double* col = part_sums + b * RS_PARTS * nq + threadIdx.x;
        double acc = col[0];
        for (int p = 1; p < RS_PARTS; ++p) acc = __dadd_rn(acc, col[(long long)p * nq]);
        sums[b * nq + threadIdx.x] = acc;
    }
    for (int i = threadIdx.x; i < nb; i += 256) {
        const int32_t* col = part_hist + b * RS_PARTS * nb + i;
        int acc = 0;
#pragma unroll 8
        for (int p = 0; p < RS_PARTS; ++p) acc += col[(long long)p * nb];
        counts[b * nb + i] = acc;
    }
    if (threadIdx.x == 255) {
        int acc = 0;
        for (int p = 0; p < RS_PARTS; ++p) acc += part_out[b * RS_PARTS + p];
        outside[b] = acc;
    }
}

struct BandEdges {
    float e[BAND_MAX_E];
};

__device__ __forceinline__ unsigned band_of(float y, const BandEdges& ed, int ne) {
    unsigned c = 0;
    for (int j = 0; j < ne; ++j) c += ed.e[j] <= y ? 1u : 0u;
    return y != y ? 255u : c;
}

// A thread takes 16 pixels: four float4 in, one 16-byte store of labels out; the last piece of an n that is no multiple of 16 goes
// element by element.
__global__ __launch_bounds__(256) void band_labels_kernel(const float* __restrict__ y, uint8_t* __restrict__ labels, long long n, BandEdges ed,
                                                          int ne) {
    const long long pieces = (n + 15) / 16;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < pieces; p += (long long)gridDim.x * blockDim.x) {
        const long long i0 = p * 16;
        if (i0 + 16 <= n) {
            const floatx4* y4 = reinterpret_cast<const floatx4*>(y + i0);
            uint4 w;
            unsigned* wp = &w.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const floatx4 yv = y4[k];
                unsigned word = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) word |= band_of(yv[e], ed, ne) << (8 * e);
                wp[k] = word;
            }
            *reinterpret_cast<uint4*>(labels + i0) = w;
        } else {
            for (long long i = i0; i < n; ++i) labels[i] = (uint8_t)band_of(y[i], ed, ne);
        }
    }
}

inline bool ranges_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

template <int S>
void launch_region_reg(const float* x, const float* tgt, const uint8_t* lab, long long bs, int L, double* ps, int32_t* ph, int32_t* po, int B,
                       long long Q, hipStream_t st) {
    hipLaunchKernelGGL(region_scores_kernel<S>, dim3(RS_PARTS, (unsigned)B), dim3(256), 0, st, x, tgt, lab, bs, L, ps, ph, po, S, Q);
}

}  // namespace

extern "C" int64_t idiff_region_scores_ws_bytes(int B, int S, int L) {
    if (B <= 0 || B > 65535 || S <= 0 || S > RS_MAX_S || L <= 0 || L > RS_MAX_L) return 0;
    return (int64_t)B * RS_PARTS * (L * RS_NQ * (int64_t)sizeof(double) + (L * (S + 2) + 1) * (int64_t)sizeof(int32_t));
}

extern "C" int idiff_region_scores(const float* x, const float* target, const uint8_t* labels, int64_t labels_bstride, int L, double* sums,
                                   int32_t* counts, int32_t* outside, void* ws, int B, int S, int64_t n_s, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && target && labels && sums && counts && outside && ws && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL,
                    "region_scores: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= RS_MAX_S, "region_scores: S = %d is outside [1, %d]", S, RS_MAX_S);
    IDIFF_CHECK_ARG(L >= 1 && L <= RS_MAX_L, "region_scores: L = %d is outside [1, %d]", L, RS_MAX_L);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "region_scores: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(labels_bstride == 0 || labels_bstride == n_s, "region_scores: labels_bstride = %lld is neither 0 nor n_s = %lld",
                    (long long)labels_bstride, (long long)n_s);
    IDIFF_CHECK_ARG(((uintptr_t)x | (uintptr_t)target) % 16 == 0, "region_scores: x and target must be 16-byte aligned");
    IDIFF_CHECK_ARG((uintptr_t)labels % 4 == 0, "region_scores: labels must be 4-byte aligned");
    IDIFF_CHECK_ARG((uintptr_t)sums % 8 == 0 && (uintptr_t)ws % 8 == 0 && (uintptr_t)counts % 4 == 0 && (uintptr_t)outside % 4 == 0,
                    "region_scores: sums and ws must be 8-byte aligned, counts and outside 4-byte aligned");
    {
        const long long nbytes[7] = {(long long)B * L * RS_NQ * 8, (long long)B * L * (S + 2) * 4, (long long)B * 4,
                                     (long long)idiff_region_scores_ws_bytes(B, S, L), (long long)B * S * n_s * 4, (long long)B * n_s * 4,
                                     (labels_bstride ? (long long)B : 1LL) * n_s};
        const void* ptr[7] = {sums, counts, outside, ws, x, target, labels};
        for (int i = 0; i < 4; ++i)  // the four buffers written, against each other and against the three read
            for (int j = i + 1; j < 7; ++j)
                IDIFF_CHECK_ARG(!ranges_overlap(ptr[i], nbytes[i], ptr[j], nbytes[j]),
                                "region_scores: sums, counts, outside and ws must be buffers of their own, apart from the inputs");
    }
    const long long Q = n_s / 4;
    hipStream_t st = (hipStream_t)stream;
    double* ps = static_cast<double*>(ws);
    int32_t* ph = reinterpret_cast<int32_t*>(ps + (long long)B * RS_PARTS * L * RS_NQ);
    int32_t* po = ph + (long long)B * RS_PARTS * L * (S + 2);
    // IDIFF_ENSEMBLE_REREAD=1 (tests): the second-read form also where the values would fit in registers, as in idiff_ensemble_scores
    const char* rr = getenv("IDIFF_ENSEMBLE_REREAD");
    if (S > RS_REG || (rr && rr[0] == '1')) {
        hipLaunchKernelGGL(region_scores_kernel<0>, dim3(RS_PARTS, (unsigned)B), dim3(256), 0, st, x, target, labels, (long long)labels_bstride, L,
                           ps, ph, po, S, Q);
    } else {
#define REGION_CASE(s)                                                                                     \
    case s:                                                                                                \
        launch_region_reg<s>(x, target, labels, (long long)labels_bstride, L, ps, ph, po, B, Q, st); \
        break;
        switch (S) {
            REGION_CASE(1) REGION_CASE(2) REGION_CASE(3) REGION_CASE(4) REGION_CASE(5) REGION_CASE(6) REGION_CASE(7) REGION_CASE(8)
            REGION_CASE(9) REGION_CASE(10) REGION_CASE(11) REGION_CASE(12) REGION_CASE(13) REGION_CASE(14) REGION_CASE(15) REGION_CASE(16)
        }
#undef REGION_CASE
    }
    IDIFF_CHECK_LAUNCH("region_scores_partial");
    hipLaunchKernelGGL(region_scores_final_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)ps, (const int32_t*)ph, (const int32_t*)po,
                       sums, counts, outside, L, S);
    IDIFF_CHECK_LAUNCH("region_scores_final");
    return IDIFF_OK;
}

extern "C" int idiff_band_labels(const float* y, uint8_t* labels, int64_t n, const float* edges_host, int ne, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(y && labels && edges_host && n > 0, "band_labels: bad args");
    IDIFF_CHECK_ARG(ne >= 1 && ne <= BAND_MAX_E, "band_labels: ne = %d is outside [1, %d]", ne, BAND_MAX_E);
    IDIFF_CHECK_ARG((uintptr_t)y % 16 == 0 && (uintptr_t)labels % 16 == 0, "band_labels: y and labels must be 16-byte aligned");
    IDIFF_CHECK_ARG(!ranges_overlap(y, (long long)n * 4, labels, (long long)n), "band_labels: labels must not overlap y");
    BandEdges ed;
    for (int j = 0; j < BAND_MAX_E; ++j) {
        ed.e[j] = j < ne ? edges_host[j] : 0.f;
        IDIFF_CHECK_ARG(j >= ne || isfinite(ed.e[j]), "band_labels: edges[%d] is not finite", j);
        IDIFF_CHECK_ARG(j == 0 || j >= ne || ed.e[j - 1] < ed.e[j], "band_labels: edges must be strictly ascending (edges[%d])", j);
    }
    const long long pieces = ((long long)n + 15) / 16;
    const long long blocks = (pieces + 255) / 256;
    hipLaunchKernelGGL(band_labels_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, y, labels,
                       (long long)n, ed, ne);
    IDIFF_CHECK_LAUNCH("band_labels");
    return IDIFF_OK;
}
