// No-reference despeckling statistics per region of a label map (include/idiff.h: idiff_despeckle_stats).  The first
// analysis kernel that needs the image geometry: it reads 4-neighbour stencils, so it knows P, H and W where the others see n_s floats.
// The object is built with -ffp-contract=off (Makefile) like region_scores.o: every fp32 operation below is rounded on its own.
//
// Launch 1, 64 x (B S) blocks of 256 threads (despeckle_stats_kernel).  Thread (p, tid) of row (b, s) takes float4 v = p*256 + tid +
// i*16384 of the row's P H W / 4 in sweep i; W % 4 == 0, so a float4 lies inside one image line: line g = v / (W/4) of the row, r = g % H
// of its plane.  Its N / S neighbours are the aligned float4 v -+ W/4 (read iff r > 0 / r < H - 1: never outside the plane, so never
// outside the row), the W / E neighbours of its end elements the scalars 4v - 1 / 4v + 4 (read iff the float4 is not the first / last of
// its line); every neighbour comes from global memory, none from another lane or sweep.  Every lane runs all ceil(Q / 16384) sweeps, a
// lane past the end with nothing to add, so every shuffle runs with 64 active lanes.  Per sweep: the four counts of a pixel's region
// (integer LDS adds, the label compared against L first); the wave's set of labels < L carried by a valid pixel (a 64-bit word, an OR
// over the xor tree, read back through readfirstlane: wave-uniform); for each label of the set and each of the 12 quantities the lane's
// fp64 sum over its elements 0 .. 3 that carry the label and count for the quantity, from +0.0; the fixed xor tree (offsets 32 .. 1);
// lane 0 adds the wave's sum to the slot [wave][label][quantity] -- sweep order.  At the end the four waves' slots are added in wave
// order: one fp64 partial per block, label and quantity.
// Launch 2, one block per row (despeckle_stats_final_kernel): adds the 64 partials of every (label, quantity) and count in index order.
// Integer LDS adds are the only atomics.
#include "common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int DS_PARTS = 64;  // partial blocks per row
constexpr int DS_MAX_S = 64;
constexpr int DS_MAX_L = 64;
constexpr int DS_NQ = 12;  // a, a^2, y, y^2, a y, rho, rho^2, La, Ly, La^2, Ly^2, La Ly
constexpr int DS_NC = 4;   // valid, ratio, stencil, invalid

__device__ __forceinline__ double ds_wave_sum_f64(double v) {  // fixed xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float ds_map(float v, float scale, float shift) { return __fadd_rn(__fmul_rn(v, scale), shift); }
__device__ __forceinline__ bool ds_finite(float v) { return fabsf(v) <= FLT_MAX; }  // false for NaN and +-inf

// The four pixels of a float4 after the per-pixel arithmetic.  kind[e]: bit 0 valid, bit 1 counted in the ratio, bit 2 in the stencil.
struct DsPix {
    floatx4 a, y, rho, la, ly;
    int kind[4];
};

// Term q of element e in fp64: the fp32 values converted first, the products formed in double (exact: two 24-bit significands).
__device__ __forceinline__ double ds_term(const DsPix& r, int q, int e) {
    switch (q) {
        case 0: return (double)r.a[e];
        case 1: return __dmul_rn((double)r.a[e], (double)r.a[e]);
        case 2: return (double)r.y[e];
        case 3: return __dmul_rn((double)r.y[e], (double)r.y[e]);
        case 4: return __dmul_rn((double)r.a[e], (double)r.y[e]);
        case 5: return (double)r.rho[e];
        case 6: return __dmul_rn((double)r.rho[e], (double)r.rho[e]);
        case 7: return (double)r.la[e];
        case 8: return (double)r.ly[e];
        case 9: return __dmul_rn((double)r.la[e], (double)r.la[e]);
        case 10: return __dmul_rn((double)r.ly[e], (double)r.ly[e]);
        default: return __dmul_rn((double)r.la[e], (double)r.ly[e]);
    }
}
__device__ __forceinline__ int ds_need(int q) { return q < 5 ? 1 : q < 7 ? 2 : 4; }  // the kind bit a quantity counts under

__global__ __launch_bounds__(256) void despeckle_stats_kernel(const float* __restrict__ x, const float* __restrict__ ref,
                                                              const uint8_t* __restrict__ labels, long long labels_bstride, int L, float scale,
                                                              float shift, float ratio_floor, double* __restrict__ part_sums,
                                                              int32_t* __restrict__ part_cnt, int32_t* __restrict__ part_out, int S, int H,
                                                              int W4, int Q) {
    __shared__ int cnt[DS_MAX_L * DS_NC];
    __shared__ double slot[4][DS_MAX_L * DS_NQ];
    __shared__ int out_lds;
    const int nq = L * DS_NQ, nc = L * DS_NC;
    for (int i = threadIdx.x; i < nc; i += 256) cnt[i] = 0;
    for (int i = threadIdx.x; i < 4 * DS_MAX_L * DS_NQ; i += 256) (&slot[0][0])[i] = 0.0;
    if (threadIdx.x == 0) out_lds = 0;
    __syncthreads();
    const long long row = blockIdx.y, b = row / S;
    const float* xr = x + row * 4 * (long long)Q;
    const float* yr = ref + b * 4 * (long long)Q;
    const floatx4* x4 = reinterpret_cast<const floatx4*>(xr);
    const floatx4* y4 = reinterpret_cast<const floatx4*>(yr);
    const uint32_t* l4 = reinterpret_cast<const uint32_t*>(labels + b * labels_bstride);
    const int lane = threadIdx.x & 63;
    double* myslot = slot[threadIdx.x >> 6];
    const int stride = DS_PARTS * 256;
    const int sweeps = (Q + stride - 1) / stride;  // the same for every lane of the grid; Q < 2^29
    int outside = 0;
    for (int i = 0; i < sweeps; ++i) {
        const int v = i * stride + (int)blockIdx.x * 256 + (int)threadIdx.x;
        int sel[4] = {-1, -1, -1, -1};  // the label of a valid pixel inside [0, L), else -1
        DsPix r;
        r.a = r.y = r.rho = r.la = r.ly = floatx4{0.f, 0.f, 0.f, 0.f};
        r.kind[0] = r.kind[1] = r.kind[2] = r.kind[3] = 0;
        unsigned long long mine = 0;
        if (v < Q) {
            const int g = v / W4, c4 = v - g * W4, rr = g % H;
            const bool hasN = rr > 0, hasS = rr < H - 1, hasW = c4 > 0, hasE = c4 < W4 - 1;
            const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
            const floatx4 xc = x4[v], yc = y4[v];
            const uint32_t lw = l4[v];
            // every neighbour read lies inside the centre's plane: v - W4 >= 0 iff r > 0, v + W4 < Q iff r < H - 1, and the scalars
            // 4v - 1 / 4v + 4 stay on the centre's line
            const floatx4 xn = hasN ? x4[v - W4] : zero, yn = hasN ? y4[v - W4] : zero;
            const floatx4 xs = hasS ? x4[v + W4] : zero, ys = hasS ? y4[v + W4] : zero;
            const float xw = hasW ? xr[4ll * v - 1] : 0.f, yw = hasW ? yr[4ll * v - 1] : 0.f;
            const float xe = hasE ? xr[4ll * v + 4] : 0.f, ye = hasE ? yr[4ll * v + 4] : 0.f;
            floatx4 an, yn_, as, ys_;
            bool okc[4], okn[4], oks[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r.a[e] = ds_map(xc[e], scale, shift);
                r.y[e] = ds_map(yc[e], scale, shift);
                an[e] = ds_map(xn[e], scale, shift);
                yn_[e] = ds_map(yn[e], scale, shift);
                as[e] = ds_map(xs[e], scale, shift);
                ys_[e] = ds_map(ys[e], scale, shift);
                okc[e] = ds_finite(r.a[e]) && ds_finite(r.y[e]);
                okn[e] = hasN && ds_finite(an[e]) && ds_finite(yn_[e]);
                oks[e] = hasS && ds_finite(as[e]) && ds_finite(ys_[e]);
            }
            const float aw = ds_map(xw, scale, shift), yw_ = ds_map(yw, scale, shift);
            const float ae = ds_map(xe, scale, shift), ye_ = ds_map(ye, scale, shift);
            const bool okw = hasW && ds_finite(aw) && ds_finite(yw_), oke = hasE && ds_finite(ae) && ds_finite(ye_);
            int pend = -1, pc[DS_NC] = {0, 0, 0, 0};  // the counts of a run of elements with one label: one LDS add per kind and run
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float aW = e == 0 ? aw : r.a[e - 1], yW = e == 0 ? yw_ : r.y[e - 1];
                const float aE = e == 3 ? ae : r.a[e + 1], yE = e == 3 ? ye_ : r.y[e + 1];
                const bool okW = e == 0 ? okw : okc[e - 1], okE = e == 3 ? oke : okc[e + 1];
                int kind = 0;
                if (okc[e]) {
                    kind = 1;
                    if (r.a[e] >= ratio_floor) {
                        kind |= 2;
                        r.rho[e] = __fdiv_rn(r.y[e], r.a[e]);
                    }
                    if (okn[e] && oks[e] && okW && okE) {
                        kind |= 4;
                        r.la[e] = __fsub_rn(__fadd_rn(__fadd_rn(an[e], as[e]), __fadd_rn(aW, aE)), __fmul_rn(4.f, r.a[e]));
                        r.ly[e] = __fsub_rn(__fadd_rn(__fadd_rn(yn_[e], ys_[e]), __fadd_rn(yW, yE)), __fmul_rn(4.f, r.y[e]));
                    }
                }
                const int lab = (int)((lw >> (8 * e)) & 0xffu);
                if (lab < L) {  // checked before it becomes an index
                    if (lab != pend) {
                        if (pend >= 0) {
#pragma unroll
                            for (int k = 0; k < DS_NC; ++k)
                                if (pc[k]) atomicAdd(&cnt[pend * DS_NC + k], pc[k]);
                        }
                        pend = lab;
                        pc[0] = pc[1] = pc[2] = pc[3] = 0;
                    }
                    pc[0] += kind & 1;
                    pc[1] += (kind >> 1) & 1;
                    pc[2] += (kind >> 2) & 1;
                    pc[3] += kind ? 0 : 1;
                    if (kind) {
                        r.kind[e] = kind;
                        sel[e] = lab;
                        mine |= 1ull << lab;
                    }
                } else {
                    ++outside;
                }
            }
            if (pend >= 0) {
#pragma unroll
                for (int k = 0; k < DS_NC; ++k)
                    if (pc[k]) atomicAdd(&cnt[pend * DS_NC + k], pc[k]);
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
            for (int q = 0; q < DS_NQ; ++q) {
                double c = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (sel[e] == l && (r.kind[e] & ds_need(q))) c = __dadd_rn(c, ds_term(r, q, e));
                c = ds_wave_sum_f64(c);
                if (lane == 0) myslot[l * DS_NQ + q] = __dadd_rn(myslot[l * DS_NQ + q], c);
            }
        }
    }
    if (outside) atomicAdd(&out_lds, outside);
    __syncthreads();  // every LDS add and every slot of the block has landed
    const long long blk = row * DS_PARTS + blockIdx.x;
    for (int t = threadIdx.x; t < nq; t += 256)  // L * 12 can exceed 256
        part_sums[blk * nq + t] = __dadd_rn(__dadd_rn(__dadd_rn(slot[0][t], slot[1][t]), slot[2][t]), slot[3][t]);
    for (int t = threadIdx.x; t < nc; t += 256) part_cnt[blk * nc + t] = cnt[t];
    if (threadIdx.x == 0) part_out[blk] = out_lds;
}

// One block per row: the 64 partials of a (label, quantity) in index order by one thread (coalesced across the threads); integer counts
// in any order give the same count.  The outside count depends on the labels alone: the row of member 0 writes it.
__global__ __launch_bounds__(256) void despeckle_stats_final_kernel(const double* __restrict__ part_sums, const int32_t* __restrict__ part_cnt,
                                                                    const int32_t* __restrict__ part_out, double* __restrict__ sums,
                                                                    int32_t* __restrict__ counts, int32_t* __restrict__ outside, int L, int S) {
    const long long row = blockIdx.x;
    const int nq = L * DS_NQ, nc = L * DS_NC;
    for (int t = threadIdx.x; t < nq; t += 256) {
        const double* col = part_sums + row * DS_PARTS * nq + t;
        double acc = col[0];
        for (int p = 1; p < DS_PARTS; ++p) acc = __dadd_rn(acc, col[(long long)p * nq]);
        sums[row * nq + t] = acc;
    }
    for (int t = threadIdx.x; t < nc; t += 256) {
        const int32_t* col = part_cnt + row * DS_PARTS * nc + t;
        int acc = 0;
#pragma unroll 8
        for (int p = 0; p < DS_PARTS; ++p) acc += col[(long long)p * nc];
        counts[row * nc + t] = acc;
    }
    if (threadIdx.x == 255 && row % S == 0) {
        int acc = 0;
        for (int p = 0; p < DS_PARTS; ++p) acc += part_out[row * DS_PARTS + p];
        outside[row / S] = acc;
    }
}

inline bool ds_ranges_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int64_t idiff_despeckle_stats_ws_bytes(int B, int S, int L) {
    if (B <= 0 || S <= 0 || S > DS_MAX_S || (long long)B * S > 65535 || L <= 0 || L > DS_MAX_L) return 0;
    return (int64_t)B * S * DS_PARTS * (L * DS_NQ * (int64_t)sizeof(double) + (L * DS_NC + 1) * (int64_t)sizeof(int32_t));
}

extern "C" int idiff_despeckle_stats(const float* x, const float* ref, const uint8_t* labels, int64_t labels_bstride, int L, float scale,
                                     float shift, float ratio_floor, double* sums, int32_t* counts, int32_t* outside, void* ws, int B, int S,
                                     int P, int H, int W, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && ref && labels && sums && counts && outside && ws && B > 0 && P > 0 && H > 0 && W > 0, "despeckle_stats: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= DS_MAX_S, "despeckle_stats: S = %d is outside [1, %d]", S, DS_MAX_S);
    IDIFF_CHECK_ARG((long long)B * S <= 65535, "despeckle_stats: B S = %lld rows are more than 65535", (long long)B * S);
    IDIFF_CHECK_ARG(L >= 1 && L <= DS_MAX_L, "despeckle_stats: L = %d is outside [1, %d]", L, DS_MAX_L);
    IDIFF_CHECK_ARG(W % 4 == 0, "despeckle_stats: W = %d is not a multiple of 4", W);
    const long long n_s = (long long)P * H * W;
    IDIFF_CHECK_ARG(n_s <= 0x7fffffffLL, "despeckle_stats: P H W = %lld is not below 2^31", n_s);
    IDIFF_CHECK_ARG(isfinite(scale) && isfinite(shift), "despeckle_stats: scale and shift must be finite");
    IDIFF_CHECK_ARG(isfinite(ratio_floor) && ratio_floor > 0.f, "despeckle_stats: ratio_floor must be finite and > 0");
    IDIFF_CHECK_ARG(labels_bstride == 0 || labels_bstride == n_s, "despeckle_stats: labels_bstride = %lld is neither 0 nor P H W = %lld",
                    (long long)labels_bstride, n_s);
    IDIFF_CHECK_ARG(((uintptr_t)x | (uintptr_t)ref) % 16 == 0, "despeckle_stats: x and ref must be 16-byte aligned");
    IDIFF_CHECK_ARG((uintptr_t)labels % 4 == 0, "despeckle_stats: labels must be 4-byte aligned");
    IDIFF_CHECK_ARG((uintptr_t)sums % 8 == 0 && (uintptr_t)ws % 8 == 0 && (uintptr_t)counts % 4 == 0 && (uintptr_t)outside % 4 == 0,
                    "despeckle_stats: sums and ws must be 8-byte aligned, counts and outside 4-byte aligned");
    {
        const long long R = (long long)B * S;
        const long long nbytes[7] = {R * L * DS_NQ * 8, R * L * DS_NC * 4, (long long)B * 4, (long long)idiff_despeckle_stats_ws_bytes(B, S, L),
                                     R * n_s * 4, (long long)B * n_s * 4, (labels_bstride ? (long long)B : 1LL) * n_s};
        const void* ptr[7] = {sums, counts, outside, ws, x, ref, labels};
        for (int i = 0; i < 4; ++i)  // the four buffers written, against each other and against the three read
            for (int j = i + 1; j < 7; ++j)
                IDIFF_CHECK_ARG(!ds_ranges_overlap(ptr[i], nbytes[i], ptr[j], nbytes[j]),
                                "despeckle_stats: sums, counts, outside and ws must be buffers of their own, apart from the inputs");
    }
    const int R = B * S, Q = (int)(n_s / 4);
    hipStream_t st = (hipStream_t)stream;
    double* ps = static_cast<double*>(ws);
    int32_t* pc = reinterpret_cast<int32_t*>(ps + (long long)R * DS_PARTS * L * DS_NQ);
    int32_t* po = pc + (long long)R * DS_PARTS * L * DS_NC;
    hipLaunchKernelGGL(despeckle_stats_kernel, dim3(DS_PARTS, (unsigned)R), dim3(256), 0, st, x, ref, labels, (long long)labels_bstride, L, scale,
                       shift, ratio_floor, ps, pc, po, S, H, W / 4, Q);
    IDIFF_CHECK_LAUNCH("despeckle_stats_partial");
    hipLaunchKernelGGL(despeckle_stats_final_kernel, dim3((unsigned)R), dim3(256), 0, st, (const double*)ps, (const int32_t*)pc,
                       (const int32_t*)po, sums, counts, outside, L, S);
    IDIFF_CHECK_LAUNCH("despeckle_stats_final");
    return IDIFF_OK;
}
