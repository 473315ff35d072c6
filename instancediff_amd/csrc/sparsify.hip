// Sparsification curves of an uncertainty map (include/idiff.h: idiff_sparsification).  Per image the K - 1 exact order
// statistics of the ranking key at the ranks floor(k N / K), and for each of them the count and the fp64 sum of the squared error
// e = (pred - target)^2 above and at the threshold.  No sort: a most-significant-digit-first radix selection of all thresholds at once,
// then fixed-order sums.  Every float operation is spelled with its rounding (__fsub_rn, __fmul_rn, __dadd_rn): the file needs no
// contraction flag.
//
// Launch 1, one block of 1024 threads per image (sparsify_select_kernel).  Pass 0 reads key / pred / target once, writes the mapped
// key u of every pixel (0 = invalid: no valid pixel maps to 0) to the workspace and fills the 256-bin histogram of u's top byte; its
// total is N, which gives the ranks m_k.  Every live threshold carries (prefix, rank inside the prefix): after a pass it scans its
// histogram from digit 255 down to the digit that holds its rank and appends it.  Thresholds are monotone in k, so their prefixes are
// sorted; equal prefixes share a histogram (at most K - 1 <= 63 of 256 int32 bins, stride 257 against bank conflicts in the scans: 63.2
// KiB of LDS).  Passes 1 .. 3 read u from the workspace (L2), find the pixel's prefix by a binary search over the distinct live
// prefixes and add 1 to its bin with an integer LDS add.  After pass 3 a prefix is the threshold itself.
// Launch 2, 64 x B x ceil(K / 8) blocks of 256 threads (sparsify_sums_kernel): a block owns (part, image, group of eight thresholds);
// a thread keeps the eight A, T sums (fp64) and c, t counts of its group at constant register indices, one compare and one predicated
// add per threshold and quantity, a thread's pixels in loop order and a float4's elements in index order; every block also adds the
// image's total.  Then idiff_ensemble_scores' reduction: the xor-shuffle tree per wave (offsets 32 .. 1), the four waves in index order.
// Launch 3, one block per image (sparsify_final_kernel): adds the 64 partials of every quantity in index order and writes the rows.
// Thresholds read back from the workspace are only compared.  Integer LDS adds are the only atomics.
#include "common.h"

#include <initializer_list>

namespace {

constexpr int SP_PARTS = 64;   // partial blocks per image and threshold group (= SCORE_PARTS)
constexpr int SP_MAX_K = 64;
constexpr int SP_GROUP = 8;    // thresholds per block of the sums launch
constexpr int SP_NQ = 2 * SP_GROUP + 1;  // fp64 quantities per block: A[8], T[8], the total
constexpr int SP_HSTRIDE = 257;          // int32 per histogram
constexpr int SP_SELECT_THREADS = 1024;
constexpr unsigned SP_DEAD = 0xffffffffu;  // the sentinel threshold: no valid pixel's u is above or at it
constexpr unsigned QNAN_BITS = 0x7fc00000u;

__host__ __device__ inline int sp_groups(int K) { return (K + SP_GROUP - 1) / SP_GROUP; }

__device__ __forceinline__ bool is_nan_bits(unsigned b) { return (b & 0x7fffffffu) > 0x7f800000u; }
// float bits -> the unsigned key whose order is the floats' (-0 and +0 tie); never 0 or 0xffffffff for a non-NaN float
__device__ __forceinline__ unsigned key_map(unsigned b) {
    if (b == 0x80000000u) b = 0u;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned key_unmap(unsigned u) { return (u >> 31) ? (u & 0x7fffffffu) : ~u; }
__device__ __forceinline__ float sq_err(float p, float t) {
    const float d = __fsub_rn(p, t);
    return __fmul_rn(d, d);
}

struct SelectState {
    unsigned prefix[SP_MAX_K];   // threshold k: the digits found so far, in place
    unsigned rank[SP_MAX_K];     // its 1-based rank among the pixels that share the prefix; 0 = no threshold (m_k = 0)
    unsigned gprefix[SP_MAX_K];  // the distinct live prefixes, descending, shifted down to the digits found so far
    int gof[SP_MAX_K];           // threshold k's histogram
    int ng;
    int nvalid;
};

// After a pass at `shift`: thread k < K walks its histogram down to its digit; then thread 0 lists the distinct prefixes for the next pass.
__device__ __forceinline__ void select_resolve(SelectState& s, const int* hist, int K, int shift) {
    const int k = threadIdx.x;
    if (k < K && s.rank[k] != 0) {
        const int* h = hist + s.gof[k] * SP_HSTRIDE;
        const unsigned r = s.rank[k];
        unsigned cum = 0, digit = 0, above = 0;
        bool found = false;
        for (int d = 255; d >= 0; --d) {
            const unsigned c = (unsigned)h[d];
            if (!found && cum + c >= r) {
                found = true;
                digit = (unsigned)d;
                above = cum;
            }
            cum += c;
        }
        s.rank[k] = r - above;
        s.prefix[k] |= digit << shift;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ng = 0;
        for (int j = 0; j < K; ++j) {
            if (s.rank[j] == 0) continue;
            const unsigned p = s.prefix[j] >> shift;
            if (ng == 0 || s.gprefix[ng - 1] != p) {
                if (ng < SP_MAX_K - 1) s.gprefix[ng++] = p;
            }
            s.gof[j] = ng - 1;
        }
        s.ng = ng;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SP_SELECT_THREADS) void sparsify_select_kernel(const float* __restrict__ key, const float* __restrict__ pred,
                                                                             const float* __restrict__ tgt, unsigned* __restrict__ ukeys,
                                                                             unsigned* __restrict__ tau_u, int32_t* __restrict__ nv,
                                                                             float* __restrict__ tau, int K, long long Q) {
    extern __shared__ int hist[];  // [SP_MAX_K - 1][SP_HSTRIDE]
    __shared__ SelectState s;
    const long long b = blockIdx.x;
    const uint4* k4 = key ? reinterpret_cast<const uint4*>(key) + b * Q : nullptr;
    const floatx4* p4 = reinterpret_cast<const floatx4*>(pred) + b * Q;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + b * Q;
    uint4* u4 = reinterpret_cast<uint4*>(ukeys) + b * Q;

    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    if (threadIdx.x < SP_MAX_K) {
        s.prefix[threadIdx.x] = 0;
        s.rank[threadIdx.x] = 0;
        s.gof[threadIdx.x] = 0;
    }
    __syncthreads();
    // pass 0: map, store, histogram of the top byte
    for (long long v = threadIdx.x; v < Q; v += blockDim.x) {
        const floatx4 p = p4[v], t = t4[v];
        unsigned kb[4];
        unsigned ev[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[e] = __float_as_uint(sq_err(p[e], t[e]));
        if (k4) {
            const uint4 kk = k4[v];
            kb[0] = kk.x, kb[1] = kk.y, kb[2] = kk.z, kb[3] = kk.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) kb[e] = ev[e];
        }
        unsigned u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = !is_nan_bits(kb[e]) && !is_nan_bits(ev[e]);
            u[e] = ok ? key_map(kb[e]) : 0u;
            if (ok) atomicAdd(&hist[u[e] >> 24], 1);
        }
        u4[v] = make_uint4(u[0], u[1], u[2], u[3]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int d = 0; d < 256; ++d) n += hist[d];
        s.nvalid = n;
    }
    __syncthreads();
    const long long N = s.nvalid;
    if ((int)threadIdx.x < K) s.rank[threadIdx.x] = (unsigned)(((long long)threadIdx.x * N) / K);  // m_k
    __syncthreads();
    select_resolve(s, hist, K, 24);
    // passes 1 .. 3: one histogram per distinct live prefix
    for (int shift = 16; shift >= 0; shift -= 8) {
        const int ng = s.ng;
        if (ng == 0) break;
        for (int i = threadIdx.x; i < ng * SP_HSTRIDE; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (long long v = threadIdx.x; v < Q; v += blockDim.x) {
            const uint4 uu = u4[v];
            const unsigned u[4] = {uu.x, uu.y, uu.z, uu.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned q = u[e] >> (shift + 8);
                int lo = 0, hi = ng;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s.gprefix[mid] > q) lo = mid + 1; else hi = mid;
                }
                if (u[e] != 0u && lo < ng && s.gprefix[lo] == q) atomicAdd(&hist[lo * SP_HSTRIDE + ((u[e] >> shift) & 255u)], 1);
            }
        }
        __syncthreads();
        select_resolve(s, hist, K, shift);
    }
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        const bool live = s.rank[k] != 0;
        tau_u[b * SP_MAX_K + k] = live ? s.prefix[k] : SP_DEAD;
        tau[b * K + k] = __uint_as_float(live ? key_unmap(s.prefix[k]) : QNAN_BITS);
    }
    if (threadIdx.x == 0) {
        nv[b * 2] = (int32_t)N;
        nv[b * 2 + 1] = (int32_t)(4 * Q - N);
    }
}

__global__ __launch_bounds__(256) void sparsify_sums_kernel(const unsigned* __restrict__ ukeys, const float* __restrict__ pred,
                                                            const float* __restrict__ tgt, const unsigned* __restrict__ tau_u,
                                                            double* __restrict__ part_sums, int32_t* __restrict__ part_counts, int K,
                                                            long long Q) {
    __shared__ double red[SP_NQ][4];
    __shared__ int redc[2 * SP_GROUP][4];
    const int part = blockIdx.x, g = blockIdx.z, G = gridDim.z;
    const long long b = blockIdx.y;
    const uint4* u4 = reinterpret_cast<const uint4*>(ukeys) + b * Q;
    const floatx4* p4 = reinterpret_cast<const floatx4*>(pred) + b * Q;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + b * Q;
    unsigned th[SP_GROUP];
#pragma unroll
    for (int j = 0; j < SP_GROUP; ++j) th[j] = g * SP_GROUP + j < K ? tau_u[b * SP_MAX_K + g * SP_GROUP + j] : SP_DEAD;
    double A[SP_GROUP], T[SP_GROUP], total = 0.0;
    int c[SP_GROUP], t[SP_GROUP];
#pragma unroll
    for (int j = 0; j < SP_GROUP; ++j) A[j] = 0.0, T[j] = 0.0, c[j] = 0, t[j] = 0;
    for (long long v = part * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)SP_PARTS * blockDim.x) {
        const uint4 uu = u4[v];
        const floatx4 p = p4[v], y = t4[v];
        const unsigned u[4] = {uu.x, uu.y, uu.z, uu.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double ed = (double)sq_err(p[e], y[e]);
            total = u[e] != 0u ? __dadd_rn(total, ed) : total;
#pragma unroll
            for (int j = 0; j < SP_GROUP; ++j) {  // an invalid pixel's u = 0 is neither above nor at any threshold
                const bool above = u[e] > th[j], at = u[e] == th[j];
                A[j] = above ? __dadd_rn(A[j], ed) : A[j];
                T[j] = at ? __dadd_rn(T[j], ed) : T[j];
                c[j] += above ? 1 : 0;
                t[j] += at ? 1 : 0;
            }
        }
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < SP_GROUP; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            A[j] = __dadd_rn(A[j], __shfl_xor(A[j], o, 64));
            T[j] = __dadd_rn(T[j], __shfl_xor(T[j], o, 64));
            c[j] += __shfl_xor(c[j], o, 64);
            t[j] += __shfl_xor(t[j], o, 64);
        }
        if (lane == 0) red[j][w] = A[j], red[SP_GROUP + j][w] = T[j], redc[j][w] = c[j], redc[SP_GROUP + j][w] = t[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total = __dadd_rn(total, __shfl_xor(total, o, 64));
    if (lane == 0) red[2 * SP_GROUP][w] = total;
    __syncthreads();
    const long long blk = (b * G + g) * SP_PARTS + part;
    if (threadIdx.x < SP_NQ) {
        const double(&r)[4] = red[threadIdx.x];
        part_sums[blk * SP_NQ + threadIdx.x] = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), r[2]), r[3]);
    }
    if (threadIdx.x < 2 * SP_GROUP) {
        const int(&r)[4] = redc[threadIdx.x];
        part_counts[blk * (2 * SP_GROUP) + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// One block per image: thread i < 2 K takes (k, column) = (i / 2, i % 2) and adds its SP_PARTS partials in index order; thread 2 K the total.
__global__ __launch_bounds__(256) void sparsify_final_kernel(const double* __restrict__ part_sums, const int32_t* __restrict__ part_counts,
                                                             const int32_t* __restrict__ nv, double* __restrict__ sums,
                                                             int32_t* __restrict__ counts, int K) {
    const long long b = blockIdx.x;
    const int G = sp_groups(K), i = threadIdx.x;
    if (i < 2 * K) {
        const int k = i >> 1, col = i & 1, g = k / SP_GROUP, q = col * SP_GROUP + k % SP_GROUP;
        const long long blk0 = (b * G + g) * SP_PARTS;
        double acc = part_sums[blk0 * SP_NQ + q];
        int n = part_counts[blk0 * (2 * SP_GROUP) + q];
        for (int p = 1; p < SP_PARTS; ++p) {
            acc = __dadd_rn(acc, part_sums[(blk0 + p) * SP_NQ + q]);
            n += part_counts[(blk0 + p) * (2 * SP_GROUP) + q];
        }
        sums[(b * (K + 1) + k) * 2 + col] = acc;
        counts[(b * (K + 1) + k) * 2 + col] = n;
    } else if (i == 2 * K) {
        const long long blk0 = b * G * SP_PARTS;  // group 0 carries the total
        double acc = part_sums[blk0 * SP_NQ + 2 * SP_GROUP];
        for (int p = 1; p < SP_PARTS; ++p) acc = __dadd_rn(acc, part_sums[(blk0 + p) * SP_NQ + 2 * SP_GROUP]);
        sums[(b * (K + 1) + K) * 2] = acc;
        sums[(b * (K + 1) + K) * 2 + 1] = 0.0;
        counts[(b * (K + 1) + K) * 2] = nv[b * 2];
        counts[(b * (K + 1) + K) * 2 + 1] = nv[b * 2 + 1];
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

// 16 bytes of slack (the mapped keys start at the first 16-byte boundary of ws), the mapped keys, then the partials and the thresholds
extern "C" int64_t idiff_sparsification_ws_bytes(int B, int K, int64_t n_s) {
    if (B <= 0 || B > 65535 || K <= 0 || K > SP_MAX_K || n_s <= 0 || n_s > 0x7fffffffLL || n_s % 4 != 0) return 0;
    const int64_t blocks = (int64_t)B * sp_groups(K) * SP_PARTS;
    return 16 + 4 * (int64_t)B * n_s + blocks * (SP_NQ * 8 + 2 * SP_GROUP * 4) + (int64_t)B * (SP_MAX_K * 4 + 8);
}

extern "C" int idiff_sparsification(const float* key, const float* pred, const float* target, int K, double* sums, int32_t* counts, float* tau,
                                    void* ws, int B, int64_t n_s, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(pred && target && sums && counts && tau && ws && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL,
                    "sparsification: bad args");
    IDIFF_CHECK_ARG(K >= 1 && K <= SP_MAX_K, "sparsification: K = %d is outside [1, %d]", K, SP_MAX_K);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "sparsification: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned_to({key, pred, target}, 16), "sparsification: key, pred and target must be 16-byte aligned");
    IDIFF_CHECK_ARG(aligned_to({sums, ws}, 8) && aligned_to({counts, tau}, 4),
                    "sparsification: sums and ws must be 8-byte aligned, counts and tau 4-byte aligned");
    const unsigned long long ib = 4ull * B * n_s, sb = 16ull * B * (K + 1), cb = 8ull * B * (K + 1), tb = 4ull * B * K,
                             wb = (unsigned long long)idiff_sparsification_ws_bytes(B, K, n_s);
    const void* bufs[] = {key, pred, target, sums, counts, tau, ws};
    const unsigned long long bytes[] = {ib, ib, ib, sb, cb, tb, wb};
    for (int i = 0; i < 7; ++i)
        for (int j = i < 3 ? 3 : i + 1; j < 7; ++j)  // the inputs may share memory with each other, never with an output
            IDIFF_CHECK_ARG(!bufs[i] || apart(bufs[i], bytes[i], bufs[j], bytes[j]),
                            "sparsification: sums, counts, tau and ws must be buffers of their own, apart from key, pred and target");
    const long long Q = n_s / 4;
    const int G = sp_groups(K);
    hipStream_t st = (hipStream_t)stream;
    unsigned* ukeys = reinterpret_cast<unsigned*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    double* ps = reinterpret_cast<double*>(ukeys + (long long)B * n_s);
    int32_t* pc = reinterpret_cast<int32_t*>(ps + (long long)B * G * SP_PARTS * SP_NQ);
    unsigned* tau_u = reinterpret_cast<unsigned*>(pc + (long long)B * G * SP_PARTS * 2 * SP_GROUP);
    int32_t* nv = reinterpret_cast<int32_t*>(tau_u + (long long)B * SP_MAX_K);
    const size_t lds = (size_t)(SP_MAX_K - 1) * SP_HSTRIDE * sizeof(int);
    static idiff_dyn_lds_cache lds_cache;
    if (const int rc = idiff_dyn_lds(lds_cache, sparsify_select_kernel, lds, "sparsification")) return rc;
    hipLaunchKernelGGL(sparsify_select_kernel, dim3((unsigned)B), dim3(SP_SELECT_THREADS), lds, st, key, pred, target, ukeys, tau_u, nv, tau, K, Q);
    IDIFF_CHECK_LAUNCH("sparsification_select");
    hipLaunchKernelGGL(sparsify_sums_kernel, dim3(SP_PARTS, (unsigned)B, (unsigned)G), dim3(256), 0, st, (const unsigned*)ukeys, pred, target,
                       (const unsigned*)tau_u, ps, pc, K, Q);
    IDIFF_CHECK_LAUNCH("sparsification_sums");
    hipLaunchKernelGGL(sparsify_final_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)ps, (const int32_t*)pc, (const int32_t*)nv, sums,
                       counts, K);
    IDIFF_CHECK_LAUNCH("sparsification_final");
    return IDIFF_OK;
}
