// Image-to-image distances between the members of a posterior ensemble, and the member picks that follow from them (include/idiff.h:
// idiff_ensemble_distances, idiff_ensemble_pick_rows).  Per image the M = S + (target != NULL) rows -- the members in
// index order, then the target -- give a symmetric M x M matrix of squared L2 distances in fp64 over the pixels at which all M rows are
// finite.  Every fp64 operation is spelled with its rounding (__dsub_rn, __fma_rn, __dadd_rn, __dsqrt_rn): the file needs no
// contraction flag.
//
// First launch, one block of 256 threads per (image, part, tile pair).  The matrix is cut into DT x DT tiles; a block owns one (part, tile
// pair ti <= tj, image) and accumulates only that tile's pairs: a thread holds DT row-i and DT row-j float4 and DT*DT fp64
// accumulators, all at constant register indices.  A diagonal tile (ti == tj) keeps the i < j half.  Rows past M in an edge tile are
// loaded from row M - 1 (an address inside the operands) and their sums are dropped by the second launch.  Validity needs all M rows:
// every block also reads the rows outside its tiles for its pixels (one compare per value; the re-reads across tile pairs come from
// L2) and replaces the values of an invalid pixel by 0, whose difference adds fma(0, 0, acc) = acc.  The blocks of tile pair 0 also
// count the valid pixels.
// Second launch, one block per image: adds the DIST_PARTS partials of every pair in index order, writes both halves of the matrix and
// the +0.0 diagonal, then scans the finished matrix (kept in LDS) for the medoid and the member nearest to the target.
#include "common.h"

#include <initializer_list>

namespace {

constexpr int DIST_PARTS = 64;  // partial blocks per image and tile pair (= SCORE_PARTS)
constexpr int DIST_MAX_S = 64;
constexpr int DIST_MAX_M = DIST_MAX_S + 1;
constexpr int DT = 8;  // tile edge in rows
constexpr int DM = 4;  // rows per batch of validity loads
constexpr unsigned QNAN_BITS = 0x7fc00000u;

__host__ __device__ inline int dist_tiles(int M) { return (M + DT - 1) / DT; }
__host__ __device__ inline int dist_tile_pairs(int M) { return dist_tiles(M) * (dist_tiles(M) + 1) / 2; }
// tile pair (ti <= tj) -> its index: the pairs of tile column tj follow those of the columns before it
__host__ __device__ inline int dist_pair_index(int ti, int tj) { return tj * (tj + 1) / 2 + ti; }

// Row r of image b as float4: a member for r < S, the target for r == S (only reached when there is one).
__device__ __forceinline__ const floatx4* dist_row(const float* __restrict__ x, const float* __restrict__ tgt, long long b, int S, int r,
                                                   long long Q) {
    return r < S ? reinterpret_cast<const floatx4*>(x) + (b * S + r) * Q : reinterpret_cast<const floatx4*>(tgt) + b * Q;
}

// The fixed xor-shuffle tree (offsets 32, 16, .. 1) over all DT*DT accumulators of a wave at once: at offset o a lane keeps the half of
// the remaining accumulators its bit o selects, hands the other half to lane ^ o and adds what it receives (own + partner's, the
// butterfly's operation, and a + b == b + a bit for bit), so 63 exchanges do the work of 64 x 6 and lane l ends with accumulator l's sum.
template <int O>
__device__ __forceinline__ void wave_sum_stage(double (&cur)[DT * DT], int lane) {
    const bool hi = lane & O;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const double keep = hi ? cur[k + O] : cur[k], send = hi ? cur[k] : cur[k + O];
        cur[k] = __dadd_rn(keep, __shfl_xor(send, O, 64));
    }
}
__device__ __forceinline__ double wave_sum_transposed(double (&cur)[DT * DT]) {
    static_assert(DT * DT == 64, "one accumulator per lane");
    const int lane = threadIdx.x & 63;
    wave_sum_stage<32>(cur, lane);
    wave_sum_stage<16>(cur, lane);
    wave_sum_stage<8>(cur, lane);
    wave_sum_stage<4>(cur, lane);
    wave_sum_stage<2>(cur, lane);
    wave_sum_stage<1>(cur, lane);
    return cur[0];
}

template <bool DIAG>
__device__ __forceinline__ void dist_tile_body(const float* __restrict__ x, const float* __restrict__ tgt, double* __restrict__ part_d2,
                                               int32_t* __restrict__ part_valid, int S, int M, long long Q, long long b, int part, int ti,
                                               int tj, double (&red)[DT * DT][4], int (&redc)[4]) {
    const floatx4* ri[DT];
    const floatx4* rj[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) {
        const int a = ti * DT + i, c = tj * DT + i;
        ri[i] = dist_row(x, tgt, b, S, a < M ? a : M - 1, Q);
        rj[i] = dist_row(x, tgt, b, S, c < M ? c : M - 1, Q);
    }
    double acc[DT * DT];
#pragma unroll
    for (int p = 0; p < DT * DT; ++p) acc[p] = 0.0;
    int nvalid = 0;
    for (long long v = part * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)DIST_PARTS * blockDim.x) {
        // the tile's rows first, so that they are in flight while the validity of the other rows is read
        floatx4 a4[DT], b4[DT];
#pragma unroll
        for (int i = 0; i < DT; ++i) {
            b4[i] = rj[i][v];
            if (!DIAG) a4[i] = ri[i][v];
        }
        // validity over all M rows: those of the other tiles DM loads at a time (past the end the last row again: a cache hit that
        // decides nothing new), then the tile's own from the registers
        bool ok[4] = {true, true, true, true};
        for (int r0 = 0; r0 < M; r0 += DM) {
            if (r0 / DT == ti || r0 / DT == tj) continue;
            floatx4 m4[DM];
#pragma unroll
            for (int u = 0; u < DM; ++u) m4[u] = dist_row(x, tgt, b, S, r0 + u < M ? r0 + u : M - 1, Q)[v];
#pragma unroll
            for (int u = 0; u < DM; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) ok[e] &= fabsf(m4[u][e]) < __builtin_inff();
        }
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ok[e] &= fabsf(b4[i][e]) < __builtin_inff();
                if (!DIAG) ok[e] &= fabsf(a4[i][e]) < __builtin_inff();
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            nvalid += ok[e] ? 1 : 0;
            double dj[DT], di[DT];
#pragma unroll
            for (int j = 0; j < DT; ++j) dj[j] = (double)(ok[e] ? b4[j][e] : 0.f);
#pragma unroll
            for (int i = 0; i < DT; ++i) di[i] = DIAG ? dj[i] : (double)(ok[e] ? a4[i][e] : 0.f);
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int j = 0; j < DT; ++j)
                    if (!DIAG || i < j) {
                        const double d = __dsub_rn(di[i], dj[j]);
                        acc[i * DT + j] = __fma_rn(d, d, acc[i * DT + j]);
                    }
        }
    }
    // wave tree (a diagonal tile's unused accumulators are zeros), then the four waves in index order: one fp64 partial per block and pair
    const int w = threadIdx.x >> 6;
    red[threadIdx.x & 63][w] = wave_sum_transposed(acc);
    int nv = nvalid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    if ((threadIdx.x & 63) == 0) redc[w] = nv;
    __syncthreads();
    const long long blk = (b * DIST_PARTS + part) * dist_tile_pairs(M) + dist_pair_index(ti, tj);
    if (threadIdx.x < DT * DT) {
        const double(&r)[4] = red[threadIdx.x];
        part_d2[blk * (DT * DT) + threadIdx.x] = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), r[2]), r[3]);
    }
    if (ti == 0 && tj == 0 && threadIdx.x == 0) part_valid[b * DIST_PARTS + part] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
}

// The grid is one-dimensional: block -> (image, part, tile pair), tile pair fastest, through xcd_remap, so that the blocks that read the
// same pixels of an image's rows run on one XCD one after the other and share its L2 (speed only: a block's result depends on its
// (image, part, tile pair) alone).
__global__ __launch_bounds__(256) void ensemble_dist_partial_kernel(const float* __restrict__ x, const float* __restrict__ tgt,
                                                                    double* __restrict__ part_d2, int32_t* __restrict__ part_valid, int S,
                                                                    int M, long long Q) {
    __shared__ double red[DT * DT][4];
    __shared__ int redc[4];
    const int ntp = dist_tile_pairs(M);
    const unsigned id = xcd_remap(blockIdx.x, gridDim.x);
    const int tp = id % ntp, part = (id / ntp) % DIST_PARTS;
    const long long b = id / ((unsigned)ntp * DIST_PARTS);
    // tp -> (ti <= tj): the inverse of dist_pair_index, by a scan over at most 9 tile columns
    int tj = 0;
    while ((tj + 1) * (tj + 2) / 2 <= tp) ++tj;
    const int ti = tp - tj * (tj + 1) / 2;
    if (ti == tj)
        dist_tile_body<true>(x, tgt, part_d2, part_valid, S, M, Q, b, part, ti, tj, red, redc);
    else
        dist_tile_body<false>(x, tgt, part_d2, part_valid, S, M, Q, b, part, ti, tj, red, redc);
}

// One block per image.  Thread t takes the pairs i < j it reaches at stride 256 and adds their DIST_PARTS partials in index order; the
// matrix also stays in LDS for the picks: one thread per member sums its row's roots in index order, thread 0 scans for the first minima.
__global__ __launch_bounds__(256) void ensemble_dist_final_kernel(const double* __restrict__ part_d2, const int32_t* __restrict__ part_valid,
                                                                  double* __restrict__ d2, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ pick, int S, int M, long long n_s) {
    __shared__ double mat[DIST_MAX_M * DIST_MAX_M];
    __shared__ double rowsum[DIST_MAX_S];
    const long long b = blockIdx.x;
    const int ntp = dist_tile_pairs(M);
    const double* base = part_d2 + b * DIST_PARTS * ntp * (DT * DT);
    double* out = d2 + b * M * M;
    for (int idx = threadIdx.x; idx < M * M; idx += blockDim.x) {
        const int i = idx / M, j = idx - i * M;
        if (i > j) continue;
        double acc = 0.0;
        if (i < j) {
            const double* p = base + (long long)dist_pair_index(i / DT, j / DT) * (DT * DT) + (i % DT) * DT + (j % DT);
            acc = p[0];
#pragma unroll 8
            for (int q = 1; q < DIST_PARTS; ++q) acc = __dadd_rn(acc, p[(long long)q * ntp * (DT * DT)]);
        }
        mat[i * M + j] = acc;
        mat[j * M + i] = acc;
        out[i * M + j] = acc;
        out[j * M + i] = acc;
    }
    if (threadIdx.x == 0) {
        int valid = 0;
        for (int q = 0; q < DIST_PARTS; ++q) valid += part_valid[b * DIST_PARTS + q];
        counts[b * 2] = valid;
        counts[b * 2 + 1] = (int32_t)(n_s - valid);
    }
    __syncthreads();
    if ((int)threadIdx.x < S) {
        const int i = threadIdx.x;
        double m = 0.0;
        for (int j = 0; j < S; ++j)
            if (j != i) m = __dadd_rn(m, __dsqrt_rn(mat[i * M + j]));
        rowsum[i] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int med = 0, best = M > S ? 0 : -1;
        for (int i = 1; i < S; ++i) {
            if (rowsum[i] < rowsum[med]) med = i;
            if (M > S && mat[i * M + S] < mat[best * M + S]) best = i;
        }
        pick[b * 2] = med;
        pick[b * 2 + 1] = best;
    }
}

// out[b] = x[b][pick[b * stride]] in 16-byte pieces; an index outside [0, S) never becomes an address: the row is quiet NaNs.
__global__ __launch_bounds__(256) void ensemble_pick_rows_kernel(const uint4* __restrict__ x, const int32_t* __restrict__ pick, int pick_stride,
                                                                 uint4* __restrict__ out, int S, long long Q) {
    const long long b = blockIdx.y;
    const int k = pick[b * pick_stride];
    const bool in_range = (unsigned)k < (unsigned)S;
    const uint4* src = x + (b * S + (in_range ? k : 0)) * Q;
    uint4* dst = out + b * Q;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x)
        dst[v] = in_range ? src[v] : make_uint4(QNAN_BITS, QNAN_BITS, QNAN_BITS, QNAN_BITS);
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

extern "C" int64_t idiff_ensemble_distances_ws_bytes(int B, int S, int has_target) {
    if (B <= 0 || B > 65535 || S <= 0 || S > DIST_MAX_S) return 0;
    const int M = S + (has_target ? 1 : 0);
    return (int64_t)B * DIST_PARTS * ((int64_t)dist_tile_pairs(M) * DT * DT * (int64_t)sizeof(double) + 8);
}

extern "C" int idiff_ensemble_distances(const float* x, const float* target, double* d2, int32_t* counts, int32_t* pick, void* ws, int B, int S,
                                        int64_t n_s, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && d2 && counts && pick && ws && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL, "ensemble_distances: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= DIST_MAX_S, "ensemble_distances: S = %d is outside [1, %d]", S, DIST_MAX_S);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_distances: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned_to({x, target}, 16), "ensemble_distances: x and target must be 16-byte aligned");
    IDIFF_CHECK_ARG(aligned_to({d2, ws}, 8) && aligned_to({counts, pick}, 4),
                    "ensemble_distances: d2 and ws must be 8-byte aligned, counts and pick 4-byte aligned");
    const int M = S + (target ? 1 : 0);
    const unsigned long long xb = 4ull * B * S * n_s, tb = target ? 4ull * B * n_s : 0, db = 8ull * B * M * M, cb = 8ull * B,
                             wb = (unsigned long long)idiff_ensemble_distances_ws_bytes(B, S, target != nullptr);
    const void* bufs[] = {x, target, d2, counts, pick, ws};
    const unsigned long long bytes[] = {xb, tb, db, cb, cb, wb};
    for (int i = 0; i < 6; ++i)
        for (int j = i < 2 ? 2 : i + 1; j < 6; ++j)  // the inputs may share memory with each other, never with an output
            IDIFF_CHECK_ARG(!bufs[i] || apart(bufs[i], bytes[i], bufs[j], bytes[j]),
                            "ensemble_distances: d2, counts, pick and ws must be buffers of their own, apart from x and target");
    const long long Q = n_s / 4;
    hipStream_t st = (hipStream_t)stream;
    const int ntp = dist_tile_pairs(M);
    double* pd = static_cast<double*>(ws);
    int32_t* pv = reinterpret_cast<int32_t*>(pd + (long long)B * DIST_PARTS * ntp * DT * DT);
    hipLaunchKernelGGL(ensemble_dist_partial_kernel, dim3((unsigned)((long long)B * DIST_PARTS * ntp)), dim3(256), 0, st, x, target, pd, pv, S, M, Q);
    IDIFF_CHECK_LAUNCH("ensemble_distances_partial");
    hipLaunchKernelGGL(ensemble_dist_final_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)pd, (const int32_t*)pv, d2, counts, pick,
                       S, M, (long long)n_s);
    IDIFF_CHECK_LAUNCH("ensemble_distances_final");
    return IDIFF_OK;
}

extern "C" int idiff_ensemble_pick_rows(const float* x, const int32_t* pick, int pick_stride, float* out, int B, int S, int64_t n_s,
                                        idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && pick && out && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL && pick_stride >= 1,
                    "ensemble_pick_rows: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= DIST_MAX_S, "ensemble_pick_rows: S = %d is outside [1, %d]", S, DIST_MAX_S);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_pick_rows: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned_to({x, out}, 16) && aligned_to({pick}, 4), "ensemble_pick_rows: x and out must be 16-byte aligned, pick 4-byte aligned");
    const unsigned long long xb = 4ull * B * S * n_s, ob = 4ull * B * n_s, pb = 4ull * ((unsigned long long)(B - 1) * pick_stride + 1);
    IDIFF_CHECK_ARG(apart(out, ob, x, xb) && apart(out, ob, pick, pb), "ensemble_pick_rows: out must not overlap x or pick");
    const long long Q = n_s / 4;
    long long gx = (Q + 255) / 256;
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(ensemble_pick_rows_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(x), pick, pick_stride, reinterpret_cast<uint4*>(out), S, Q);
    IDIFF_CHECK_LAUNCH("ensemble_pick_rows");
    return IDIFF_OK;
}
