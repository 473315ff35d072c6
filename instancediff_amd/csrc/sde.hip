// SDE update kernels: fused reverse steps (IRSDE and driftSDE), Philox4x32-10 normals, per-sample mixes.
// HBM-bound streaming kernels (float4 per lane).  The IRSDE step reproduces the reference's fp32 operation
// order exactly (utils/sde_utils.py:45-46,178-188): every product / sum below is rounded once, no FMA
// contraction, IEEE division, so with injected noise the result is bit-identical to the CPU reference.
#include "common.h"

#include <cstdlib>
#include <initializer_list>
#include <utility>

// hipcc defaults to -ffp-contract=fast-honor-pragmas: without this the separate mul/sub below fuse to FMAs
// and the result differs from the reference's op-by-op fp32 arithmetic in the last bit.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f + 2.98023223876953125e-8f; }  // (0,1)

// 4 standard normals for counter ctr (Box-Muller on word pairs).  member fills the upper 64 counter bits: 0 is the library's one
// stream, m >= 1 the noise stream of ensemble member m (disjoint from stream 0 and from every other member at any ctr).
__device__ __forceinline__ floatx4 philox_normal4(uint64_t ctr, uint64_t seed, uint64_t member = 0) {
    uint32_t w[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)member, (uint32_t)(member >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const float r0 = sqrtf(-2.0f * logf(u01(w[0])));
    const float r1 = sqrtf(-2.0f * logf(u01(w[2])));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u01(w[1]), &s0, &c0);
    sincosf(6.283185307179586f * u01(w[3]), &s1, &c1);
    floatx4 z = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
    return z;
}

__device__ __forceinline__ floatx4 ld4(const float* p, long long i, long long n) {
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
    if (i + 3 < n) return *reinterpret_cast<const floatx4*>(p + i);
    for (int k = 0; k < 4; ++k)
        if (i + k < n) v[k] = p[i + k];
    return v;
}
__device__ __forceinline__ void st4(float* p, long long i, long long n, floatx4 v) {
    if (i + 3 < n) {
        *reinterpret_cast<floatx4*>(p + i) = v;
        return;
    }
    for (int k = 0; k < 4; ++k)
        if (i + k < n) p[i + k] = v[k];
}

template <int MODE>
__global__ __launch_bounds__(256) void irsde_step_kernel(const float* __restrict__ x, const float* __restrict__ mu, const float* __restrict__ np_,
                                                         const float* __restrict__ z, float* __restrict__ xo, long long n, float theta,
                                                         float sigma, float sigma_bar, float dt, float sqrt_dt, uint64_t seed,
                                                         uint64_t offset) {
    const float s2 = __fmul_rn(sigma, sigma);
    const float coef = MODE == IDIFF_SDE_ODE ? __fmul_rn(0.5f, s2) : s2;
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
        const long long i = v * 4;
        const floatx4 xv = ld4(x, i, n), mv = ld4(mu, i, n), nv4 = ld4(np_, i, n);
        floatx4 zv = {0.f, 0.f, 0.f, 0.f};
        if (MODE == IDIFF_SDE_STEP) zv = z ? ld4(z, i, n) : philox_normal4(offset + (uint64_t)v, seed);
        floatx4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // correctly rounded fp32 quotient: an fp64 divide rounded to fp32 is exact for p=24 (53 >= 2p+2),
            // independent of how the compiler lowers fp32 division by a loop-invariant scalar.
            const float score = (float)((double)(-nv4[k]) / (double)sigma_bar);
            const float t1 = __fsub_rn(mv[k], xv[k]);
            const float t2 = __fmul_rn(theta, t1);
            const float t3 = __fmul_rn(coef, score);
            const float t4 = __fsub_rn(t2, t3);
            const float t5 = __fmul_rn(t4, dt);
            float r = __fsub_rn(xv[k], t5);
            if (MODE == IDIFF_SDE_STEP) {
                const float nz = __fmul_rn(zv[k], sqrt_dt);
                r = __fsub_rn(r, __fmul_rn(sigma, nz));
            }
            o[k] = r;
        }
        st4(xo, i, n, o);
    }
}

// ---- the driftSDE reverse update ----
// Each piece of the update is defined once, here; the drift_step*_kernel forms below differ only in where their operands live.  Every
// operation is rounded once, in the order written.
struct StepCoef {
    float a, b, c, rho_d, rho_s;
    bool hist_d, hist_s;
};

// Row t = state[0] of coef [3][Tp1] = (a, b, c), or with HIST of coef [5][Tp1] = (a, b, c, rho_d, rho_s); without HIST rows 3-4 are never
// read.  A rho != 0 turns that clock's history on -- true for NaN too: an off-schedule row poisons the result.
template <bool HIST>
__device__ __forceinline__ StepCoef load_step_coef(const float* __restrict__ coef, int Tp1, const int* __restrict__ state) {
    const int t = state[0];
    StepCoef k = {coef[t], coef[Tp1 + t], coef[2 * Tp1 + t], 0.f, 0.f, false, false};
    if (HIST) {
        k.rho_d = coef[3 * Tp1 + t];
        k.rho_s = coef[4 * Tp1 + t];
        k.hist_d = k.rho_d != 0.f;
        k.hist_s = k.rho_s != 0.f;
    }
    return k;
}

// r + rho*(r - prev): one clock's prediction extrapolated linearly from the previous jump's
__device__ __forceinline__ floatx4 extrapolate(floatx4 r, floatx4 prev, float rho) {
    floatx4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __fadd_rn(r[k], __fmul_rn(rho, __fsub_rn(r[k], prev[k])));
    return o;
}

// z of one 4-element group: zero where c == 0 (nothing is read or drawn), injected() -- the form's load of its group of the injected
// noise -- when there is a noise base, otherwise the Philox normals of (ctr, member)
template <class Load>
__device__ __forceinline__ floatx4 step_noise(float c, bool have_base, Load injected, uint64_t ctr, uint64_t seed, uint64_t member = 0) {
    floatx4 zv = {0.f, 0.f, 0.f, 0.f};
    if (c != 0.f) zv = have_base ? injected() : philox_normal4(ctr, seed, member);
    return zv;
}

// o = ((x - a*R) - b*e) + c*z,  oa = o - cond
__device__ __forceinline__ void step_update(floatx4 xv, floatx4 rt, floatx4 et, floatx4 zv, floatx4 cv, float a, float b, float c, floatx4& o,
                                            floatx4& oa) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float r = __fsub_rn(xv[k], __fmul_rn(a, rt[k]));
        r = __fsub_rn(r, __fmul_rn(b, et[k]));
        r = __fadd_rn(r, __fmul_rn(c, zv[k]));
        o[k] = r;
        oa[k] = __fsub_rn(r, cv[k]);
    }
}

__global__ __launch_bounds__(256) void drift_step_kernel(const float* __restrict__ x, const float* __restrict__ rh, const float* __restrict__ eh,
                                                         const float* __restrict__ z, const float* __restrict__ cond, float* __restrict__ xo,
                                                         float* __restrict__ xao, long long n, float a, float b, float c, uint64_t seed,
                                                         uint64_t offset) {
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
        const long long i = v * 4;
        const floatx4 xv = ld4(x, i, n), rv = ld4(rh, i, n), ev = ld4(eh, i, n);
        const floatx4 zv = step_noise(c, z != nullptr, [&] { return ld4(z, i, n); }, offset + (uint64_t)v, seed);
        floatx4 o, oa;
        floatx4 cv = {0.f, 0.f, 0.f, 0.f};
        if (xao) cv = ld4(cond, i, n);
        step_update(xv, rv, ev, zv, cv, a, b, c, o, oa);
        st4(xo, i, n, o);
        if (xao) st4(xao, i, n, oa);
    }
}

// Graph-replayable form of the drift step: every per-step scalar comes from device memory, so ONE captured HIP graph of a
// denoising step replays for every t.  state = {t, Philox call count, step index of this run}; coef = [3][Tp1] tables of
// (a_t, b_t, c_t); injected noise (parity runs) is indexed by the step index.  In place: x <- update, xa <- x - cond
// (element-wise, each thread reads before it writes its own element).
// HIST is the second-order multistep form (driftSDE solver_order = 2): coef = [5][Tp1] tables of (a, b, c, rho_d, rho_s); each
// prediction is extrapolated linearly from the previous jump's, kept in rp / ep at fixed addresses for the next replay:
//   R~ = r + rho_d*(r - rp),  e~ = e + rho_s*(e - ep),  x <- ((x - a*R~) - b*e~) + c*z,  xa <- x - cond,  rp <- r,  ep <- e.
// rho_d, rho_s are uniform over the grid.  A zero rho skips that clock's history read and its term (the first jump of a chain, a
// flat level table), so with both zero the arithmetic is the 3-row form's whatever rp / ep hold.  Without HIST rp / ep are not touched.
template <bool HIST>
__global__ __launch_bounds__(256) void drift_step_dev_kernel(float* x, const float* __restrict__ rh, const float* __restrict__ eh, float* rp,
                                                             float* ep, const float* __restrict__ zbase, const float* __restrict__ cond,
                                                             float* xa, long long n, const float* __restrict__ coef, int Tp1,
                                                             const int* __restrict__ state, uint64_t seed, uint64_t nper,
                                                             uint64_t offset_base) {
    const StepCoef k = load_step_coef<HIST>(coef, Tp1, state);
    const uint64_t offset = offset_base + (uint64_t)(unsigned)state[1] * nper;
    const float* z = zbase ? zbase + (long long)state[2] * n : nullptr;
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
        const long long i = v * 4;
        const floatx4 xv = ld4(x, i, n), rv = ld4(rh, i, n), ev = ld4(eh, i, n);
        floatx4 rt = rv, et = ev;
        if (k.hist_d) rt = extrapolate(rv, ld4(rp, i, n), k.rho_d);
        if (k.hist_s) et = extrapolate(ev, ld4(ep, i, n), k.rho_s);
        const floatx4 zv = step_noise(k.c, z != nullptr, [&] { return ld4(z, i, n); }, offset + (uint64_t)v, seed);
        const floatx4 cv = ld4(cond, i, n);
        floatx4 o, oa;
        step_update(xv, rt, et, zv, cv, k.a, k.b, k.c, o, oa);
        st4(x, i, n, o);
        st4(xa, i, n, oa);
        if (HIST) {
            st4(rp, i, n, rv);
            st4(ep, i, n, ev);
        }
    }
}

// t <- t-1 (wrapping to T below t_stop+1, for benchmark loops), counters += 1, tdev[:] = t  -- the host never touches a
// per-step scalar between graph replays
__global__ void step_state_advance_kernel(int* state, float* tdev, int B, int T, int t_stop) {
    int t = state[0] - 1;
    if (t <= t_stop) t = T;
    for (int i = threadIdx.x; i < B; i += blockDim.x) tdev[i] = (float)t;
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = t;
        state[1] += 1;
        state[2] += 1;
    }
}

// Few-step form: t <- next_t[t] along a host-built schedule t_0 > t_1 > ... > t_K = 0 (wrapping to t_first once t <= t_stop),
// counters += 1, tdev[:] = t.  A t outside [0, Tp1), read or produced, restarts at t_first: next_t is never read out of bounds.
__global__ void step_state_advance_table_kernel(int* state, float* tdev, int B, const int* __restrict__ next_t, int Tp1, int t_first,
                                                int t_stop) {
    const int cur = state[0];
    int t = (cur >= 0 && cur < Tp1) ? next_t[cur] : t_first;
    if (t <= t_stop || t >= Tp1) t = t_first;
    for (int i = threadIdx.x; i < B; i += blockDim.x) tdev[i] = (float)t;
    __syncthreads();
    if (threadIdx.x == 0) {
        state[0] = t;
        state[1] += 1;
        state[2] += 1;
    }
}

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long long n, uint64_t seed, uint64_t offset) {
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x)
        st4(out, v * 4, n, philox_normal4(offset + (uint64_t)v, seed));
}

// Inverted dropout keyed by the Philox stream: element i is kept iff the 24 high bits of word i % 4 of counter offset + i / 4,
// as u in [0, 1), are >= p; kept elements are scaled by 1 / (1 - p).  The mask is a pure function of (seed, offset, i): the backward
// pass applies the same launch to the gradient instead of storing a mask.
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float p, float scale,
                                                      uint64_t seed, uint64_t offset) {
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
        uint32_t w[4];
        const uint64_t ctr = offset + (uint64_t)v;
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = v * 4 + k;
            if (i < n) {
                const float u = (float)(w[k] >> 8) * (1.0f / 16777216.0f);
                out[i] = u >= p ? __fmul_rn(x[i], scale) : 0.f;
            }
        }
    }
}

__global__ void philox_raw_kernel(uint32_t* __restrict__ out, long long nc, uint64_t seed, uint64_t offset) {
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nc; v += (long long)gridDim.x * blockDim.x) {
        uint32_t w[4];
        const uint64_t ctr = offset + (uint64_t)v;
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        for (int k = 0; k < 4; ++k) out[v * 4 + k] = w[k];
    }
}

__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, long long n,
                                                    float alpha, float beta) {
    const long long nv = (n + 3) / 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
        const long long i = v * 4;
        const floatx4 xv = ld4(x, i, n), yv = ld4(y, i, n);
        floatx4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __fadd_rn(__fmul_rn(alpha, xv[k]), __fmul_rn(beta, yv[k]));
        st4(out, i, n, o);
    }
}

__global__ __launch_bounds__(256) void mix3_kernel(const float* __restrict__ x0, const float* __restrict__ cond, const float* __restrict__ eps,
                                                   const float* __restrict__ c0, const float* __restrict__ c1, const float* __restrict__ c2,
                                                   float* __restrict__ out, long long per) {
    const int b = blockIdx.y;
    const float a0 = c0[b], a1 = c1[b], a2 = c2[b];
    const long long base = (long long)b * per;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        float r = __fmul_rn(a0, x0[base + i]);
        r = __fadd_rn(r, __fmul_rn(a1, cond[base + i]));
        r = __fadd_rn(r, __fmul_rn(a2, eps[base + i]));
        out[base + i] = r;
    }
}


// ---- IRSDE pieces (idiff_irsde_map): the reference's own decomposition of its steps and closed forms, one launch each ----
struct IrsdeCoef {
    float k[6];
};

template <int OP>
__device__ __forceinline__ float irsde_piece(float a, float b, float z, float m, const float* k) {
    if (OP == IDIFF_IRSDE_SCORE_FROM_NOISE) return (float)((double)(-a) / (double)k[0]);  // correctly rounded fp32 quotient
    if (OP == IDIFF_IRSDE_MU_BAR) return __fadd_rn(m, __fmul_rn(__fsub_rn(a, m), k[0]));
    if (OP == IDIFF_IRSDE_DRIFT) return __fmul_rn(__fmul_rn(k[0], __fsub_rn(m, a)), k[1]);
    if (OP == IDIFF_IRSDE_DISPERSION) return __fmul_rn(k[0], __fmul_rn(z, k[1]));
    if (OP == IDIFF_IRSDE_REV_DRIFT || OP == IDIFF_IRSDE_STEP_MEAN || OP == IDIFF_IRSDE_STEP_SDE) {
        const float rd = __fmul_rn(__fsub_rn(__fmul_rn(k[0], __fsub_rn(m, a)), __fmul_rn(k[1], b)), k[2]);
        if (OP == IDIFF_IRSDE_REV_DRIFT) return rd;
        const float r = __fsub_rn(a, rd);
        if (OP == IDIFF_IRSDE_STEP_MEAN) return r;
        return __fsub_rn(r, __fmul_rn(k[3], __fmul_rn(z, k[4])));
    }
    if (OP == IDIFF_IRSDE_FORWARD_STEP)
        return __fadd_rn(__fadd_rn(a, __fmul_rn(__fmul_rn(k[0], __fsub_rn(m, a)), k[1])), __fmul_rn(k[3], __fmul_rn(z, k[4])));
    if (OP == IDIFF_IRSDE_OPT_STEP)
        return __fadd_rn(__fadd_rn(__fmul_rn(k[0], __fsub_rn(a, m)), __fmul_rn(k[1], __fsub_rn(b, m))), m);
    if (OP == IDIFF_IRSDE_REAL_NOISE || OP == IDIFF_IRSDE_REAL_SCORE) {
        const float d = __fsub_rn(a, __fadd_rn(m, __fmul_rn(__fsub_rn(b, m), k[0])));
        return (float)((double)(OP == IDIFF_IRSDE_REAL_SCORE ? -d : d) / (double)k[1]);
    }
    if (OP == IDIFF_IRSDE_INIT_FROM_NOISE) return __fadd_rn(__fmul_rn(__fsub_rn(__fsub_rn(a, m), __fmul_rn(k[0], b)), k[1]), m);
    if (OP == IDIFF_IRSDE_RANDOM_STATES) return __fadd_rn(__fmul_rn(z, k[1]), __fadd_rn(m, __fmul_rn(__fsub_rn(a, m), k[0])));
    return 0.f;
}

constexpr bool irsde_op_draws(int op) {
    return op == IDIFF_IRSDE_DISPERSION || op == IDIFF_IRSDE_STEP_SDE || op == IDIFF_IRSDE_FORWARD_STEP || op == IDIFF_IRSDE_RANDOM_STATES;
}

// grid = (chunks, B); per % 4 == 0 -> float4 lanes, Philox counter = offset + (flat element index)/4 as in idiff_randn
template <int OP>
__global__ __launch_bounds__(256) void irsde_map_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ z,
                                                        const float* __restrict__ mu, float mu_scalar, float* __restrict__ out, long long per,
                                                        const float* __restrict__ coef_dev, IrsdeCoef kc, uint64_t seed, uint64_t offset, int vec4) {
    const int s = blockIdx.y;
    float k[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = coef_dev ? coef_dev[s * 6 + i] : kc.k[i];
    const long long base = (long long)s * per;
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    const floatx4 mconst = {mu_scalar, mu_scalar, mu_scalar, mu_scalar};
    if (vec4) {  // per % 4 == 0 and every operand 16-byte aligned (checked on the host)
        const long long nv = per / 4;
        for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
            const long long i = base + v * 4;
            const floatx4 av = a ? *reinterpret_cast<const floatx4*>(a + i) : zero;
            const floatx4 bv = b ? *reinterpret_cast<const floatx4*>(b + i) : zero;
            const floatx4 mv = mu ? *reinterpret_cast<const floatx4*>(mu + i) : mconst;
            floatx4 zv = zero;
            if (irsde_op_draws(OP)) zv = z ? *reinterpret_cast<const floatx4*>(z + i) : philox_normal4(offset + (uint64_t)(i >> 2), seed);
            floatx4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = irsde_piece<OP>(av[e], bv[e], zv[e], mv[e], k);
            *reinterpret_cast<floatx4*>(out + i) = o;
        }
    } else {
        for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < per; j += (long long)gridDim.x * blockDim.x) {
            const long long i = base + j;
            float zz = 0.f;
            if (irsde_op_draws(OP)) zz = z ? z[i] : philox_normal4(offset + (uint64_t)(i >> 2), seed)[i & 3];
            out[i] = irsde_piece<OP>(a ? a[i] : 0.f, b ? b[i] : 0.f, zz, mu ? mu[i] : mu_scalar, k);
        }
    }
}

template <int OP>
void launch_irsde_map(const float* a, const float* b, const float* z, const float* mu, float mu_scalar, float* out, int B, long long per,
                      const float* coef_dev, const IrsdeCoef& kc, uint64_t seed, uint64_t offset, hipStream_t st) {
    long long gx = ((per + 3) / 4 + 255) / 256;
    if (gx < 1) gx = 1;
    if (gx > 1024) gx = 1024;
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)z | (uintptr_t)mu | (uintptr_t)out;
    const int vec4 = (per % 4 == 0) && (bits % 16 == 0);
    hipLaunchKernelGGL(irsde_map_kernel<OP>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, a, b, z, mu, mu_scalar, out, per, coef_dev, kc, seed,
                       offset, vec4);
}

// ---- posterior ensembles: member noise streams (include/idiff.h) ----
// Every kernel below runs on rows of n_s = 4*Q elements, grid = (chunks, rows), 16-byte aligned operands (checked on the host).
// Row r belongs to member members[r]; its draw j uses Philox counters (j*Q + v, member) for the 4-element group v of the row:
// nothing about a member's noise depends on the row it sits in, on the other rows, or on earlier draws of the generator.
__global__ __launch_bounds__(256) void randn_members_kernel(float* __restrict__ out, long long Q, const uint64_t* __restrict__ members,
                                                            uint64_t seed, uint64_t j) {
    const uint64_t m = members[blockIdx.y];
    floatx4* o = reinterpret_cast<floatx4*>(out) + (long long)blockIdx.y * Q;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x)
        o[v] = philox_normal4(j * (uint64_t)Q + (uint64_t)v, seed, m);
}

// the start of a chain from a cond group and its x_T draw:  x = 1*cond + sigma*z,  xa = x - cond  (axpby's products by 1 and -1 are exact)
__device__ __forceinline__ void chain_start4(floatx4 cv, floatx4 zv, float sigma, floatx4& o, floatx4& oa) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[k] = __fadd_rn(cv[k], __fmul_rn(sigma, zv[k]));
        oa[k] = __fsub_rn(o[k], cv[k]);
    }
}

// output row `row` of a member chain's start from cond row `src`: cond_rep = cond, x and xa from member m's draw j = 0 (chain_start4)
__device__ __forceinline__ void member_row_start(const float* __restrict__ cond, float* __restrict__ cond_rep, float* __restrict__ x,
                                                 float* __restrict__ xa, long long src, long long row, long long Q, uint64_t m, float sigma,
                                                 uint64_t seed) {
    const floatx4* c = reinterpret_cast<const floatx4*>(cond) + src * Q;
    floatx4* cr = reinterpret_cast<floatx4*>(cond_rep) + row * Q;
    floatx4* xo = reinterpret_cast<floatx4*>(x) + row * Q;
    floatx4* xao = reinterpret_cast<floatx4*>(xa) + row * Q;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        const floatx4 cv = c[v], zv = philox_normal4((uint64_t)v, seed, m);
        floatx4 o, oa;
        chain_start4(cv, zv, sigma, o, oa);
        cr[v] = cv;
        xo[v] = o;
        xao[v] = oa;
    }
}

// row b*S + s:  cond_rep = cond[b],  x = 1*cond + sigma*z(member, j = 0),  xa = x - cond
__global__ __launch_bounds__(256) void ensemble_init_kernel(const float* __restrict__ cond, float* __restrict__ cond_rep, float* __restrict__ x,
                                                            float* __restrict__ xa, int S, long long Q, const uint64_t* __restrict__ members,
                                                            float sigma, uint64_t seed) {
    const long long row = blockIdx.y;
    member_row_start(cond, cond_rep, x, xa, row / S, row, Q, members[row], sigma, seed);
}

// The start of an image in a held chain (idiff_chain_begin): the x_T construction into the chain's own buffers plus the device state
// of its first step, in one launch.  MEMBERS: grid (chunks, R), output row r is ensemble row row0 + r (member_row_start); otherwise a
// flat grid over the n elements of the batch with the plain stream's counters offset + v, tail by ld4 / st4 as in randn_kernel.
// Block (0, 0) also writes state = {t0, calls0, 0} and tdev[0..R) = t0; no block of this launch reads either.
template <bool MEMBERS>
__global__ __launch_bounds__(256) void chain_begin_kernel(const float* __restrict__ cond_in, float* __restrict__ cond, float* __restrict__ x,
                                                          float* __restrict__ xa, long long n, int S, long long Q, long long row0, int R,
                                                          const uint64_t* __restrict__ members, float sigma, uint64_t seed, uint64_t offset,
                                                          int* __restrict__ state, float* __restrict__ tdev, int t0, int calls0) {
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int i = threadIdx.x; i < R; i += blockDim.x) tdev[i] = (float)t0;
        if (threadIdx.x < 3) state[threadIdx.x] = threadIdx.x == 0 ? t0 : (threadIdx.x == 1 ? calls0 : 0);
    }
    if (MEMBERS) {
        const long long row = blockIdx.y;
        member_row_start(cond_in, cond, x, xa, (row0 + row) / S, row, Q, members[row], sigma, seed);
    } else {
        const long long nv = (n + 3) / 4;
        for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nv; v += (long long)gridDim.x * blockDim.x) {
            const long long i = v * 4;
            const floatx4 cv = ld4(cond_in, i, n), zv = philox_normal4(offset + (uint64_t)v, seed);
            floatx4 o, oa;
            chain_start4(cv, zv, sigma, o, oa);
            st4(cond, i, n, cv);
            st4(x, i, n, o);
            st4(xa, i, n, oa);
        }
    }
}

// drift_step_dev_kernel<HIST> on rows: the z of row r is drawn from its member's stream at draw index j = 1 + state[1].
template <bool HIST>
__global__ __launch_bounds__(256) void drift_step_members_kernel(float* x, const float* __restrict__ rh, const float* __restrict__ eh, float* rp,
                                                                 float* ep, const float* __restrict__ zbase, const float* __restrict__ cond,
                                                                 float* xa, long long Q, const float* __restrict__ coef, int Tp1,
                                                                 const int* __restrict__ state, const uint64_t* __restrict__ members,
                                                                 uint64_t seed) {
    const StepCoef k = load_step_coef<HIST>(coef, Tp1, state);
    const uint64_t m = members[blockIdx.y];
    const uint64_t q0 = (1ull + (uint64_t)(unsigned)state[1]) * (uint64_t)Q;
    const long long row0 = (long long)blockIdx.y * Q;  // in 4-element groups
    const floatx4* z = zbase ? reinterpret_cast<const floatx4*>(zbase) + (long long)state[2] * ((long long)gridDim.y * Q) + row0 : nullptr;
    floatx4* xv4 = reinterpret_cast<floatx4*>(x) + row0;
    floatx4* xa4 = reinterpret_cast<floatx4*>(xa) + row0;
    const floatx4* r4 = reinterpret_cast<const floatx4*>(rh) + row0;
    const floatx4* e4 = reinterpret_cast<const floatx4*>(eh) + row0;
    const floatx4* c4 = reinterpret_cast<const floatx4*>(cond) + row0;
    floatx4* rp4 = HIST ? reinterpret_cast<floatx4*>(rp) + row0 : nullptr;
    floatx4* ep4 = HIST ? reinterpret_cast<floatx4*>(ep) + row0 : nullptr;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        const floatx4 xv = xv4[v], rv = r4[v], ev = e4[v];
        floatx4 rt = rv, et = ev;
        if (k.hist_d) rt = extrapolate(rv, rp4[v], k.rho_d);
        if (k.hist_s) et = extrapolate(ev, ep4[v], k.rho_s);
        const floatx4 zv = step_noise(k.c, z != nullptr, [&] { return z[v]; }, q0 + (uint64_t)v, seed, m);
        const floatx4 cv = c4[v];
        floatx4 o, oa;
        step_update(xv, rt, et, zv, cv, k.a, k.b, k.c, o, oa);
        xv4[v] = o;
        xa4[v] = oa;
        if (HIST) {
            rp4[v] = rv;
            ep4[v] = ev;
        }
    }
}

// Per-pixel mean and sample standard deviation over the S members of an image, members in index order, one rounding per operation:
//   mean = (..((x_0 + x_1) + x_2)..) / S,   std = sqrt((..((d_0^2 + d_1^2) + d_2^2)..) / (S - 1)),  d_s = x_s - mean   (std = 0 for S = 1).
// REG keeps a thread's S <= ENS_REG float4 values in registers between the two sums; otherwise they are read a second time.  Both do
// the same operations in the same order.  Quotients and the root go through fp64 and are rounded to fp32 (correctly rounded, as in
// irsde_step_kernel).
constexpr int ENS_REG = 16;
template <bool REG>
__global__ __launch_bounds__(256) void ensemble_stats_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ sd, int S,
                                                             long long Q) {
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    floatx4* mo = reinterpret_cast<floatx4*>(mean) + (long long)blockIdx.y * Q;
    floatx4* so = reinterpret_cast<floatx4*>(sd) + (long long)blockIdx.y * Q;
    const double dS = (double)S, dS1 = (double)(S - 1);
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        floatx4 val[REG ? ENS_REG : 1];
        floatx4 acc = xs[v];
        if (REG) {
            val[0] = acc;
#pragma unroll
            for (int s = 1; s < ENS_REG; ++s)
                if (s < S) val[s] = xs[(long long)s * Q + v];
#pragma unroll
            for (int s = 1; s < ENS_REG; ++s)
                if (s < S)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], val[s][k]);
        } else {
            for (int s = 1; s < S; ++s) {
                const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], xv[k]);
            }
        }
        floatx4 mv, ss = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) mv[k] = (float)((double)acc[k] / dS);
        if (REG) {
#pragma unroll
            for (int s = 0; s < ENS_REG; ++s)
                if (s < S)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float d = __fsub_rn(val[s][k], mv[k]);
                        ss[k] = s == 0 ? __fmul_rn(d, d) : __fadd_rn(ss[k], __fmul_rn(d, d));
                    }
        } else {
            for (int s = 0; s < S; ++s) {
                const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = __fsub_rn(xv[k], mv[k]);
                    ss[k] = s == 0 ? __fmul_rn(d, d) : __fadd_rn(ss[k], __fmul_rn(d, d));
                }
            }
        }
        if (S > 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sv[k] = (float)sqrt((double)(float)((double)ss[k] / dS1));  // fp64 sqrt of an fp32 value, rounded once more: correctly rounded
        }
        mo[v] = mv;
        so[v] = sv;
    }
}

// ---- tiled sampling (driftSDE tile / tile_overlap) ----
// The state is ONE full-resolution image [B][C][H][W]; the nets see it as a batch of Ph x Pw windows, row ((b*ny + iy)*nx + ix).
// Per axis of length L the host plan gives an int32 table {first[L], cov_lo[L], cov_hi[L], origin[n]} and an fp32 table {w0[L], w1[L]}:
// first = the lower of the (at most two, adjacent) windows with non-zero blend weight at a coordinate, w0 / w1 their weights, and
// [cov_lo, cov_hi) the windows whose extent holds the coordinate.  W, Pw and the W origins are multiples of 4, so a float4 group
// never straddles a window edge and `first` and the coverage are uniform over it.
struct TileGeom {
    int C, H, W4, ny, nx, Ph, Pw4;
    const int* yi;    // first | cov_lo | cov_hi | origin, over H
    const int* xi;    // the same over W (element coordinates)
    const float* yw;  // w0 | w1 over H
    const float* xw;  // w0 | w1 over W
};

// float4 index inside the tile buffers of pixel group (bc = b*C + c, y, x4) seen from window (iy, ix)
__device__ __forceinline__ long long tile_at(const TileGeom& g, long long b, int c, int y, int x4, int iy, int ix) {
    const int H = g.H, W = g.W4 * 4;
    const int ly = y - g.yi[3 * H + iy], lx4 = x4 - (g.xi[3 * W + ix] >> 2);
    return ((((b * g.ny + iy) * g.nx + ix) * g.C + c) * g.Ph + ly) * g.Pw4 + lx4;
}

__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ full, float* __restrict__ tiles, long long nvt, TileGeom g) {
    const floatx4* f4 = reinterpret_cast<const floatx4*>(full);
    floatx4* t4 = reinterpret_cast<floatx4*>(tiles);
    const int H = g.H, W = g.W4 * 4;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < nvt; v += (long long)gridDim.x * blockDim.x) {
        const long long trow = v / g.Pw4;
        const int lx4 = (int)(v - trow * g.Pw4);
        const long long tc = trow / g.Ph;
        const int ly = (int)(trow - tc * g.Ph);
        const long long win = tc / g.C;
        const int c = (int)(tc - win * g.C);
        const long long by = win / g.nx;
        const int ix = (int)(win - by * g.nx);
        const long long b = by / g.ny;
        const int iy = (int)(by - b * g.ny);
        const int y = g.yi[3 * H + iy] + ly, x4 = (g.xi[3 * W + ix] >> 2) + lx4;
        t4[v] = f4[((b * g.C + c) * H + y) * g.W4 + x4];
    }
}

// One slot of the blend: acc = w*r for the first term of an element, acc + w*r after it; an element whose weight is exactly 0 takes
// nothing from the slot, and a slot whose four weights are all 0 is not read.
__device__ __forceinline__ void blend_slot(const floatx4* __restrict__ src, long long at, float wy, floatx4 wx, floatx4& acc, bool (&have)[4]) {
    floatx4 w;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = __fmul_rn(wy, wx[k]);
    if (w[0] == 0.f && w[1] == 0.f && w[2] == 0.f && w[3] == 0.f) return;
    const floatx4 rv = src[at];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (w[k] == 0.f) continue;
        const float p = __fmul_rn(w[k], rv[k]);
        acc[k] = have[k] ? __fadd_rn(acc[k], p) : p;
        have[k] = true;
    }
}

// The tiled step.  Per float4 group v of the full image: blend the windows' predictions into R^ and e^ (slots (iy0,ix0), (iy0,ix1),
// (iy1,ix0), (iy1,ix1) in that order, weight wy*wx), extrapolate them when HIST, draw z at the plain chain's counter offset + v,
// update (the shared pieces above, as drift_step_dev_kernel<HIST>), and scatter x and x - cond into every window whose extent holds
// the group.  Element-wise per pixel: a thread reads and writes only its own group of x / rp / ep and of each window's copy of it.
// MEMBERS is the same step on the rows of an ensemble (idiff_drift_reverse_step_tiled_members_dev): grid = (chunks, R), nv = Q is the
// groups of ONE row, block row r works on groups r*Q + vl of the R-row image, and its z is drawn as drift_step_members_kernel draws it,
// from member members[r]'s stream at counter (1 + state[1])*Q + vl; nper and offset_base are not read.  Nothing else differs.
template <bool HIST, bool MEMBERS>
__global__ __launch_bounds__(256) void drift_step_tiled_kernel(float* x, const float* __restrict__ rt_, const float* __restrict__ et_, float* rp,
                                                               float* ep, const float* __restrict__ zbase, const float* __restrict__ cond,
                                                               float* __restrict__ xt_, float* __restrict__ xat_, long long nv, TileGeom g,
                                                               const float* __restrict__ coef, int Tp1, const int* __restrict__ state,
                                                               uint64_t seed, uint64_t nper, uint64_t offset_base,
                                                               const uint64_t* __restrict__ members) {
    const StepCoef k = load_step_coef<HIST>(coef, Tp1, state);
    const uint64_t offset = MEMBERS ? (1ull + (uint64_t)(unsigned)state[1]) * (uint64_t)nv : offset_base + (uint64_t)(unsigned)state[1] * nper;
    const uint64_t m = MEMBERS ? members[blockIdx.y] : 0;
    const long long v0 = MEMBERS ? (long long)blockIdx.y * nv : 0;                // the row's first group in the image
    const long long nimg = MEMBERS ? (long long)gridDim.y * nv : nv;              // groups of the whole image: one step of z_base
    const floatx4* z4 = zbase ? reinterpret_cast<const floatx4*>(zbase) + (long long)state[2] * nimg : nullptr;
    floatx4* x4p = reinterpret_cast<floatx4*>(x);
    const floatx4* c4 = reinterpret_cast<const floatx4*>(cond);
    const floatx4* r4 = reinterpret_cast<const floatx4*>(rt_);
    const floatx4* e4 = reinterpret_cast<const floatx4*>(et_);
    floatx4* xt4 = reinterpret_cast<floatx4*>(xt_);
    floatx4* xat4 = reinterpret_cast<floatx4*>(xat_);
    floatx4* rp4 = reinterpret_cast<floatx4*>(rp);
    floatx4* ep4 = reinterpret_cast<floatx4*>(ep);
    const int H = g.H, W = g.W4 * 4;
    for (long long vl = blockIdx.x * (long long)blockDim.x + threadIdx.x; vl < nv; vl += (long long)gridDim.x * blockDim.x) {
        const long long v = v0 + vl;
        const long long row = v / g.W4;
        const int xg = (int)(v - row * g.W4);
        const long long bc = row / H;
        const int y = (int)(row - bc * H);
        const long long bi = bc / g.C;
        const int ci = (int)(bc - bi * g.C);
        const int xe = xg * 4;
        const int iy0 = g.yi[y], ix0 = g.xi[xe];
        const float wy0 = g.yw[y], wy1 = g.yw[H + y];
        const floatx4 wx0 = *reinterpret_cast<const floatx4*>(g.xw + xe), wx1 = *reinterpret_cast<const floatx4*>(g.xw + W + xe);
        const bool y1 = wy1 != 0.f;
        const bool x1 = wx1[0] != 0.f || wx1[1] != 0.f || wx1[2] != 0.f || wx1[3] != 0.f;
        // a slot without weight may name a window that does not exist (first + 1 == n): its address is never formed
        const long long a00 = tile_at(g, bi, ci, y, xg, iy0, ix0);
        const long long a01 = x1 ? tile_at(g, bi, ci, y, xg, iy0, ix0 + 1) : 0;
        const long long a10 = y1 ? tile_at(g, bi, ci, y, xg, iy0 + 1, ix0) : 0;
        const long long a11 = (y1 && x1) ? tile_at(g, bi, ci, y, xg, iy0 + 1, ix0 + 1) : 0;
        const floatx4 zero4 = {0.f, 0.f, 0.f, 0.f};
        floatx4 rv = zero4, ev = zero4;
        {
            bool have[4] = {false, false, false, false};
            blend_slot(r4, a00, wy0, wx0, rv, have);
            if (x1) blend_slot(r4, a01, wy0, wx1, rv, have);
            if (y1) blend_slot(r4, a10, wy1, wx0, rv, have);
            if (y1 && x1) blend_slot(r4, a11, wy1, wx1, rv, have);
        }
        {
            bool have[4] = {false, false, false, false};
            blend_slot(e4, a00, wy0, wx0, ev, have);
            if (x1) blend_slot(e4, a01, wy0, wx1, ev, have);
            if (y1) blend_slot(e4, a10, wy1, wx0, ev, have);
            if (y1 && x1) blend_slot(e4, a11, wy1, wx1, ev, have);
        }
        const floatx4 xv = x4p[v];
        floatx4 rt = rv, et = ev;
        if (k.hist_d) rt = extrapolate(rv, rp4[v], k.rho_d);
        if (k.hist_s) et = extrapolate(ev, ep4[v], k.rho_s);
        const floatx4 zv = step_noise(k.c, z4 != nullptr, [&] { return z4[v]; }, offset + (uint64_t)vl, seed, m);
        const floatx4 cv = c4[v];
        floatx4 o, oa;
        step_update(xv, rt, et, zv, cv, k.a, k.b, k.c, o, oa);
        x4p[v] = o;
        if (HIST) {
            rp4[v] = rv;
            ep4[v] = ev;
        }
        const int cy0 = g.yi[H + y], cy1 = g.yi[2 * H + y], cx0 = g.xi[W + xe], cx1 = g.xi[2 * W + xe];
        for (int iy = cy0; iy < cy1; ++iy)
            for (int ix = cx0; ix < cx1; ++ix) {
                const long long at = tile_at(g, bi, ci, y, xg, iy, ix);
                xt4[at] = o;
                xat4[at] = oa;
            }
    }
}

inline int stream_grid(long long nvec) {
    long long g = (nvec + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > 2048 ? 2048 : g);
}

// The history buffers of a 5-row step are read and rewritten element by element beside `others`, the operands the step reads or writes
// at other addresses: they must be distinct from each other and from each of those.
inline bool history_distinct(const float* r_prev, const float* e_prev, std::initializer_list<const void*> others) {
    if (r_prev == e_prev) return false;
    for (const void* p : others)
        if (p == r_prev || p == e_prev) return false;
    return true;
}

// coef_rows (3 or 5, checked by the caller) = 3 takes no history buffers, 5 needs both
inline int check_coef_rows(const char* who, int coef_rows, const float* r_prev, const float* e_prev) {
    IDIFF_CHECK_ARG(coef_rows == 5 || (!r_prev && !e_prev), "%s: coef_rows = 3 takes no history buffers", who);
    IDIFF_CHECK_ARG(coef_rows == 3 || (r_prev && e_prev), "%s: coef_rows = 5 needs the history buffers", who);
    return IDIFF_OK;
}

}  // namespace

extern "C" int idiff_irsde_reverse_step(const float* x, const float* mu, const float* noise_pred, const float* z, float* x_out, int64_t n,
                                        float theta, float sigma, float sigma_bar, float dt, float sqrt_dt, int mode, uint64_t seed,
                                        uint64_t offset, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && mu && noise_pred && x_out && n > 0, "irsde_reverse_step: bad args");
    IDIFF_CHECK_ARG(mode >= 0 && mode <= 2, "irsde_reverse_step: bad mode %d", mode);
    IDIFF_CHECK_ARG(sigma_bar != 0.f, "irsde_reverse_step: sigma_bar == 0");
    const int grid = stream_grid((n + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
    if (mode == IDIFF_SDE_STEP)
        hipLaunchKernelGGL(irsde_step_kernel<IDIFF_SDE_STEP>, dim3(grid), dim3(256), 0, st, x, mu, noise_pred, z, x_out, (long long)n, theta,
                           sigma, sigma_bar, dt, sqrt_dt, seed, offset);
    else if (mode == IDIFF_SDE_MEAN)
        hipLaunchKernelGGL(irsde_step_kernel<IDIFF_SDE_MEAN>, dim3(grid), dim3(256), 0, st, x, mu, noise_pred, z, x_out, (long long)n, theta,
                           sigma, sigma_bar, dt, sqrt_dt, seed, offset);
    else
        hipLaunchKernelGGL(irsde_step_kernel<IDIFF_SDE_ODE>, dim3(grid), dim3(256), 0, st, x, mu, noise_pred, z, x_out, (long long)n, theta,
                           sigma, sigma_bar, dt, sqrt_dt, seed, offset);
    IDIFF_CHECK_LAUNCH("irsde_reverse_step");
    return IDIFF_OK;
}


extern "C" int idiff_irsde_map(int op, const float* a, const float* b, const float* z, const float* mu, float mu_scalar, float* out, int B,
                               int64_t per_sample, const float* coef_dev, const float* k, uint64_t seed, uint64_t offset, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(op >= 0 && op < IDIFF_IRSDE_NUM_OPS, "irsde_map: bad op %d", op);
    IDIFF_CHECK_ARG(out && B > 0 && B <= 65535 && per_sample > 0, "irsde_map: bad args");
    IDIFF_CHECK_ARG(coef_dev || k, "irsde_map: needs coefficients (coef_dev or k)");
    IDIFF_CHECK_ARG(a || op == IDIFF_IRSDE_DISPERSION, "irsde_map: op %d reads operand a", op);
    const bool needs_b = op == IDIFF_IRSDE_REV_DRIFT || op == IDIFF_IRSDE_STEP_MEAN || op == IDIFF_IRSDE_STEP_SDE || op == IDIFF_IRSDE_OPT_STEP ||
                         op == IDIFF_IRSDE_REAL_NOISE || op == IDIFF_IRSDE_REAL_SCORE || op == IDIFF_IRSDE_INIT_FROM_NOISE;
    IDIFF_CHECK_ARG(b || !needs_b, "irsde_map: op %d reads operand b", op);
    IrsdeCoef kc;
    for (int i = 0; i < 6; ++i) kc.k[i] = k ? k[i] : 0.f;
    if (!coef_dev && (op == IDIFF_IRSDE_SCORE_FROM_NOISE || op == IDIFF_IRSDE_REAL_NOISE || op == IDIFF_IRSDE_REAL_SCORE))
        IDIFF_CHECK_ARG(kc.k[op == IDIFF_IRSDE_SCORE_FROM_NOISE ? 0 : 1] != 0.f, "irsde_map: division by sigma_bar == 0");
    hipStream_t st = (hipStream_t)stream;
    const long long per = (long long)per_sample;
#define IDIFF_IRSDE_CASE(OP)                                                                           \
    case OP:                                                                                           \
        launch_irsde_map<OP>(a, b, z, mu, mu_scalar, out, B, per, coef_dev, kc, seed, offset, st); \
        break;
    switch (op) {
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_SCORE_FROM_NOISE)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_MU_BAR)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_DRIFT)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_REV_DRIFT)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_DISPERSION)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_STEP_MEAN)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_STEP_SDE)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_FORWARD_STEP)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_OPT_STEP)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_REAL_NOISE)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_REAL_SCORE)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_INIT_FROM_NOISE)
        IDIFF_IRSDE_CASE(IDIFF_IRSDE_RANDOM_STATES)
    }
#undef IDIFF_IRSDE_CASE
    IDIFF_CHECK_LAUNCH("irsde_map");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step(const float* x, const float* r_hat, const float* e_hat, const float* z, const float* cond, float* x_out,
                                        float* xa_out, int64_t n, float a, float b, float c, uint64_t seed, uint64_t offset,
                                        idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && r_hat && e_hat && x_out && n > 0, "drift_reverse_step: bad args");
    IDIFF_CHECK_ARG(!xa_out || cond, "drift_reverse_step: xa_out needs cond");
    hipLaunchKernelGGL(drift_step_kernel, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, r_hat, e_hat, z, cond, x_out,
                       xa_out, (long long)n, a, b, c, seed, offset);
    IDIFF_CHECK_LAUNCH("drift_reverse_step");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step_dev(float* x, const float* r_hat, const float* e_hat, const float* z_base, const float* cond, float* xa,
                                            int64_t n, const float* coef, int Tp1, const int32_t* state, uint64_t seed, uint64_t nper,
                                            uint64_t offset_base, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && r_hat && e_hat && cond && xa && coef && state && n > 0 && Tp1 > 1, "drift_reverse_step_dev: bad args");
    hipLaunchKernelGGL(drift_step_dev_kernel<false>, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, r_hat, e_hat,
                       (float*)nullptr, (float*)nullptr, z_base, cond, xa, (long long)n, coef, Tp1, state, seed, nper, offset_base);
    IDIFF_CHECK_LAUNCH("drift_reverse_step_dev");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step2_dev(float* x, const float* r_hat, const float* e_hat, float* r_prev, float* e_prev, const float* z_base,
                                             const float* cond, float* xa, int64_t n, const float* coef5, int Tp1, const int32_t* state,
                                             uint64_t seed, uint64_t nper, uint64_t offset_base, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && r_hat && e_hat && r_prev && e_prev && cond && xa && coef5 && state && n > 0 && Tp1 > 1,
                    "drift_reverse_step2_dev: bad args");
    IDIFF_CHECK_ARG(history_distinct(r_prev, e_prev, {r_hat, e_hat, x, xa}),
                    "drift_reverse_step2_dev: the history buffers must be distinct from each other and from every other operand");
    hipLaunchKernelGGL(drift_step_dev_kernel<true>, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, r_hat, e_hat, r_prev,
                       e_prev, z_base, cond, xa, (long long)n, coef5, Tp1, state, seed, nper, offset_base);
    IDIFF_CHECK_LAUNCH("drift_reverse_step2_dev");
    return IDIFF_OK;
}

extern "C" int idiff_step_state_advance(int32_t* state, float* tdev, int B, int T, int t_stop, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(state && tdev && B > 0 && T > 0 && t_stop >= 0 && t_stop < T, "step_state_advance: bad args");
    hipLaunchKernelGGL(step_state_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, tdev, B, T, t_stop);
    IDIFF_CHECK_LAUNCH("step_state_advance");
    return IDIFF_OK;
}

extern "C" int idiff_step_state_advance_table(int32_t* state, float* tdev, int B, const int32_t* next_t, int Tp1, int t_first, int t_stop,
                                              idiff_stream_t stream) {
    IDIFF_CHECK_ARG(state && tdev && next_t && B > 0 && Tp1 > 1 && t_first > 0 && t_first < Tp1 && t_stop >= 0 && t_stop < t_first,
                    "step_state_advance_table: bad args");
    hipLaunchKernelGGL(step_state_advance_table_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, tdev, B, next_t, Tp1, t_first, t_stop);
    IDIFF_CHECK_LAUNCH("step_state_advance_table");
    return IDIFF_OK;
}

extern "C" int idiff_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(out && n > 0, "randn: bad args");
    hipLaunchKernelGGL(randn_kernel, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, (long long)n, seed, offset);
    IDIFF_CHECK_LAUNCH("randn");
    return IDIFF_OK;
}

extern "C" int idiff_dropout(const float* x, float* out, int64_t n, float p, uint64_t seed, uint64_t offset, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && out && n > 0 && p >= 0.f && p < 1.f, "dropout: bad args (p must be in [0, 1))");
    hipLaunchKernelGGL(dropout_kernel, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n, p, 1.0f / (1.0f - p),
                       seed, offset);
    IDIFF_CHECK_LAUNCH("dropout");
    return IDIFF_OK;
}

extern "C" int idiff_philox_raw(uint32_t* out, int64_t ncounters, uint64_t seed, uint64_t offset, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(out && ncounters > 0, "philox_raw: bad args");
    hipLaunchKernelGGL(philox_raw_kernel, dim3(stream_grid(ncounters)), dim3(256), 0, (hipStream_t)stream, out, (long long)ncounters, seed,
                       offset);
    IDIFF_CHECK_LAUNCH("philox_raw");
    return IDIFF_OK;
}

extern "C" int idiff_axpby(const float* x, const float* y, float* out, int64_t n, float alpha, float beta, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && y && out && n > 0, "axpby: bad args");
    hipLaunchKernelGGL(axpby_kernel, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, out, (long long)n, alpha, beta);
    IDIFF_CHECK_LAUNCH("axpby");
    return IDIFF_OK;
}

extern "C" int idiff_mix3_per_sample(const float* x0, const float* cond, const float* eps, const float* c0, const float* c1, const float* c2,
                                     float* out, int B, int64_t per_sample, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x0 && cond && eps && c0 && c1 && c2 && out && B > 0 && per_sample > 0, "mix3_per_sample: bad args");
    dim3 grid(stream_grid(per_sample), B);
    hipLaunchKernelGGL(mix3_kernel, grid, dim3(256), 0, (hipStream_t)stream, x0, cond, eps, c0, c1, c2, out, (long long)per_sample);
    IDIFF_CHECK_LAUNCH("mix3_per_sample");
    return IDIFF_OK;
}

// ---- posterior ensembles ----
namespace {
inline bool aligned16(std::initializer_list<const void*> ps) {
    uintptr_t bits = 0;
    for (const void* p : ps) bits |= (uintptr_t)p;
    return bits % 16 == 0;
}
inline dim3 rows_grid(long long Q, long long rows) {  // enough blocks over all rows to fill the device, at most 2048 per row
    long long gx = (Q + 255) / 256;
    if (gx > 2048) gx = 2048;
    return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)rows);
}
}  // namespace

// ---- tiled sampling ----
namespace {
inline bool tile_geom(TileGeom& g, int B, int C, int H, int W, int ny, int nx, int Ph, int Pw, const int32_t* ytab, const float* ywt,
                      const int32_t* xtab, const float* xwt, bool weights = true) {
    if (!(ytab && xtab && (!weights || (ywt && xwt)) && B > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && Ph > 0 && Pw > 0)) return false;
    if (W % 4 || Pw % 4 || Ph > H || Pw > W || (ny == 1) != (Ph == H) || (nx == 1) != (Pw == W)) return false;
    if ((long long)ny * Ph < H || (long long)nx * Pw < W) return false;  // the windows cannot cover the image
    g = TileGeom{C, H, W / 4, ny, nx, Ph, Pw / 4, ytab, xtab, ywt, xwt};
    return true;
}
}  // namespace

extern "C" int idiff_tile_gather(const float* full, float* tiles, int B, int C, int H, int W, int ny, int nx, int Ph, int Pw,
                                 const int32_t* ytab, const int32_t* xtab, idiff_stream_t stream) {
    TileGeom g;
    IDIFF_CHECK_ARG(full && tiles && full != tiles && tile_geom(g, B, C, H, W, ny, nx, Ph, Pw, ytab, nullptr, xtab, nullptr, false),
                    "tile_gather: bad args (W, Pw multiples of 4; windows inside and covering the image)");
    IDIFF_CHECK_ARG(aligned16({full, tiles}), "tile_gather: operands must be 16-byte aligned");
    const long long nvt = (long long)B * ny * nx * C * Ph * (Pw / 4);
    hipLaunchKernelGGL(tile_gather_kernel, dim3(stream_grid(nvt)), dim3(256), 0, (hipStream_t)stream, full, tiles, nvt, g);
    IDIFF_CHECK_LAUNCH("tile_gather");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step_tiled_dev(float* x, const float* r_tiles, const float* e_tiles, float* r_prev, float* e_prev,
                                                  const float* z_base, const float* cond, float* x_tiles, float* xa_tiles, int B, int C, int H,
                                                  int W, int ny, int nx, int Ph, int Pw, const int32_t* ytab, const float* ywt,
                                                  const int32_t* xtab, const float* xwt, const float* coef, int coef_rows, int Tp1,
                                                  const int32_t* state, uint64_t seed, uint64_t nper, uint64_t offset_base,
                                                  idiff_stream_t stream) {
    TileGeom g;
    IDIFF_CHECK_ARG(x && r_tiles && e_tiles && cond && x_tiles && xa_tiles && coef && state && Tp1 > 1 &&
                        tile_geom(g, B, C, H, W, ny, nx, Ph, Pw, ytab, ywt, xtab, xwt),
                    "drift_reverse_step_tiled_dev: bad args (W, Pw multiples of 4; windows inside and covering the image)");
    IDIFF_CHECK_ARG(coef_rows == 3 || coef_rows == 5, "drift_reverse_step_tiled_dev: coef_rows must be 3 or 5, got %d", coef_rows);
    IDIFF_CHECK_ARG(aligned16({x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, xwt}),
                    "drift_reverse_step_tiled_dev: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(x_tiles != xa_tiles && x_tiles != r_tiles && x_tiles != e_tiles && xa_tiles != r_tiles && xa_tiles != e_tiles &&
                        x != x_tiles && x != xa_tiles && x != r_tiles && x != e_tiles && x != cond,
                    "drift_reverse_step_tiled_dev: the image and the four window buffers must be distinct");
    if (const int rc = check_coef_rows("drift_reverse_step_tiled_dev", coef_rows, r_prev, e_prev)) return rc;
    IDIFF_CHECK_ARG(coef_rows == 3 || history_distinct(r_prev, e_prev, {r_tiles, e_tiles, x, x_tiles, xa_tiles}),
                    "drift_reverse_step_tiled_dev: the history buffers must be distinct from each other and from every other operand");
    const long long nv = (long long)B * C * H * (W / 4);
    hipLaunchKernelGGL((coef_rows == 3 ? drift_step_tiled_kernel<false, false> : drift_step_tiled_kernel<true, false>), dim3(stream_grid(nv)),
                       dim3(256), 0, (hipStream_t)stream, x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, nv, g, coef, Tp1,
                       state, seed, nper, offset_base, (const uint64_t*)nullptr);
    IDIFF_CHECK_LAUNCH("drift_reverse_step_tiled_dev");
    return IDIFF_OK;
}

extern "C" int idiff_randn_members(float* out, int R, int64_t n_s, const uint64_t* members_dev, uint64_t seed, uint64_t j,
                                   idiff_stream_t stream) {
    IDIFF_CHECK_ARG(out && members_dev && R > 0 && R <= 65535 && n_s > 0, "randn_members: bad args");
    IDIFF_CHECK_ARG(n_s % 4 == 0, "randn_members: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({out}), "randn_members: out must be 16-byte aligned");
    hipLaunchKernelGGL(randn_members_kernel, rows_grid(n_s / 4, R), dim3(256), 0, (hipStream_t)stream, out, (long long)(n_s / 4), members_dev, seed,
                       j);
    IDIFF_CHECK_LAUNCH("randn_members");
    return IDIFF_OK;
}

extern "C" int idiff_ensemble_init(const float* cond, float* cond_rep, float* x, float* xa, int B, int S, int64_t n_s,
                                   const uint64_t* members_dev, float sigma, uint64_t seed, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(cond && cond_rep && x && xa && members_dev && B > 0 && S > 0 && (long long)B * S <= 65535 && n_s > 0,
                    "ensemble_init: bad args");
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_init: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({cond, cond_rep, x, xa}), "ensemble_init: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(cond_rep != x && cond_rep != xa && x != xa && cond != cond_rep && cond != x && cond != xa,
                    "ensemble_init: operands must be distinct");
    hipLaunchKernelGGL(ensemble_init_kernel, rows_grid(n_s / 4, (long long)B * S), dim3(256), 0, (hipStream_t)stream, cond, cond_rep, x, xa, S,
                       (long long)(n_s / 4), members_dev, sigma, seed);
    IDIFF_CHECK_LAUNCH("ensemble_init");
    return IDIFF_OK;
}

extern "C" int idiff_chain_begin(const float* cond_in, float* cond, float* x, float* xa, int B, int S, int64_t n_s, int64_t row0, int R,
                                 const uint64_t* members_dev, float sigma, uint64_t seed, uint64_t offset, int32_t* state, float* tdev, int t0,
                                 int calls0, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(cond_in && cond && x && xa && state && tdev && B > 0 && S > 0 && n_s > 0 && R > 0 && R <= 65535 && t0 >= 0 && calls0 >= 0,
                    "chain_begin: bad args");
    IDIFF_CHECK_ARG(aligned16({cond_in, cond, x, xa}), "chain_begin: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(cond != x && cond != xa && x != xa && cond_in != cond && cond_in != x && cond_in != xa,
                    "chain_begin: cond_in and the three outputs must be distinct");
    if (!members_dev) {
        IDIFF_CHECK_ARG(S == 1 && row0 == 0 && R == B, "chain_begin: the plain chain takes S = 1, row0 = 0, R = B (got S = %d, row0 = %lld, R = %d, B = %d)",
                        S, (long long)row0, R, B);
        const long long n = (long long)B * n_s;
        hipLaunchKernelGGL(chain_begin_kernel<false>, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, cond_in, cond, x, xa, n, 1,
                           0ll, 0ll, R, members_dev, sigma, seed, offset, state, tdev, t0, calls0);
    } else {
        IDIFF_CHECK_ARG(n_s % 4 == 0, "chain_begin: n_s = %lld is not a multiple of 4", (long long)n_s);
        IDIFF_CHECK_ARG(row0 >= 0 && row0 + R <= (long long)B * S, "chain_begin: rows [%lld, %lld) are not rows of the %d x %d ensemble",
                        (long long)row0, (long long)row0 + R, B, S);
        hipLaunchKernelGGL(chain_begin_kernel<true>, rows_grid(n_s / 4, R), dim3(256), 0, (hipStream_t)stream, cond_in, cond, x, xa, 0ll, S,
                           (long long)(n_s / 4), (long long)row0, R, members_dev, sigma, seed, offset, state, tdev, t0, calls0);
    }
    IDIFF_CHECK_LAUNCH("chain_begin");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step_members_dev(float* x, const float* r_hat, const float* e_hat, float* r_prev, float* e_prev,
                                                    const float* z_base, const float* cond, float* xa, int R, int64_t n_s, const float* coef,
                                                    int coef_rows, int Tp1, const int32_t* state, const uint64_t* members_dev, uint64_t seed,
                                                    idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && r_hat && e_hat && cond && xa && coef && state && members_dev && R > 0 && R <= 65535 && n_s > 0 && Tp1 > 1,
                    "drift_reverse_step_members_dev: bad args");
    IDIFF_CHECK_ARG(coef_rows == 3 || coef_rows == 5, "drift_reverse_step_members_dev: coef_rows must be 3 or 5, got %d", coef_rows);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "drift_reverse_step_members_dev: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({x, r_hat, e_hat, r_prev, e_prev, z_base, cond, xa}),
                    "drift_reverse_step_members_dev: operands must be 16-byte aligned");
    if (const int rc = check_coef_rows("drift_reverse_step_members_dev", coef_rows, r_prev, e_prev)) return rc;
    IDIFF_CHECK_ARG(coef_rows == 3 || history_distinct(r_prev, e_prev, {r_hat, e_hat, x, xa}),
                    "drift_reverse_step_members_dev: the history buffers must be distinct from each other and from every other operand");
    const long long Q = n_s / 4;
    hipLaunchKernelGGL(coef_rows == 3 ? drift_step_members_kernel<false> : drift_step_members_kernel<true>, rows_grid(Q, R), dim3(256), 0,
                       (hipStream_t)stream, x, r_hat, e_hat, r_prev, e_prev, z_base, cond, xa, Q, coef, Tp1, state, members_dev, seed);
    IDIFF_CHECK_LAUNCH("drift_reverse_step_members_dev");
    return IDIFF_OK;
}

extern "C" int idiff_drift_reverse_step_tiled_members_dev(float* x, const float* r_tiles, const float* e_tiles, float* r_prev, float* e_prev,
                                                          const float* z_base, const float* cond, float* x_tiles, float* xa_tiles, int R, int C,
                                                          int H, int W, int ny, int nx, int Ph, int Pw, const int32_t* ytab, const float* ywt,
                                                          const int32_t* xtab, const float* xwt, const float* coef, int coef_rows, int Tp1,
                                                          const int32_t* state, const uint64_t* members_dev, uint64_t seed,
                                                          idiff_stream_t stream) {
    TileGeom g;
    IDIFF_CHECK_ARG(x && r_tiles && e_tiles && cond && x_tiles && xa_tiles && coef && state && members_dev && Tp1 > 1 && R > 0 && R <= 65535 &&
                        tile_geom(g, R, C, H, W, ny, nx, Ph, Pw, ytab, ywt, xtab, xwt),
                    "drift_reverse_step_tiled_members_dev: bad args (0 < R <= 65535; W, Pw multiples of 4; windows inside and covering the image)");
    IDIFF_CHECK_ARG(coef_rows == 3 || coef_rows == 5, "drift_reverse_step_tiled_members_dev: coef_rows must be 3 or 5, got %d", coef_rows);
    IDIFF_CHECK_ARG(aligned16({x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, xwt}),
                    "drift_reverse_step_tiled_members_dev: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(x_tiles != xa_tiles && x_tiles != r_tiles && x_tiles != e_tiles && xa_tiles != r_tiles && xa_tiles != e_tiles &&
                        x != x_tiles && x != xa_tiles && x != r_tiles && x != e_tiles && x != cond,
                    "drift_reverse_step_tiled_members_dev: the image and the four window buffers must be distinct");
    if (const int rc = check_coef_rows("drift_reverse_step_tiled_members_dev", coef_rows, r_prev, e_prev)) return rc;
    IDIFF_CHECK_ARG(coef_rows == 3 || history_distinct(r_prev, e_prev, {r_tiles, e_tiles, x, x_tiles, xa_tiles}),
                    "drift_reverse_step_tiled_members_dev: the history buffers must be distinct from each other and from every other operand");
    const long long Q = (long long)C * H * (W / 4);
    hipLaunchKernelGGL((coef_rows == 3 ? drift_step_tiled_kernel<false, true> : drift_step_tiled_kernel<true, true>), rows_grid(Q, R), dim3(256),
                       0, (hipStream_t)stream, x, r_tiles, e_tiles, r_prev, e_prev, z_base, cond, x_tiles, xa_tiles, Q, g, coef, Tp1, state, seed,
                       (uint64_t)0, (uint64_t)0, members_dev);
    IDIFF_CHECK_LAUNCH("drift_reverse_step_tiled_members_dev");
    return IDIFF_OK;
}

extern "C" int idiff_ensemble_stats(const float* x, float* mean, float* std_out, int B, int S, int64_t n_s, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && mean && std_out && B > 0 && B <= 65535 && S > 0 && n_s > 0, "ensemble_stats: bad args");
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_stats: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({x, mean, std_out}), "ensemble_stats: operands must be 16-byte aligned");
    const long long Q = n_s / 4;
    // IDIFF_ENSEMBLE_REREAD=1 (tests): the second-read form also where the values would fit in registers
    const char* rr = getenv("IDIFF_ENSEMBLE_REREAD");
    const bool reg = S <= ENS_REG && !(rr && rr[0] == '1');
    if (reg)
        hipLaunchKernelGGL(ensemble_stats_kernel<true>, rows_grid(Q, B), dim3(256), 0, (hipStream_t)stream, x, mean, std_out, S, Q);
    else
        hipLaunchKernelGGL(ensemble_stats_kernel<false>, rows_grid(Q, B), dim3(256), 0, (hipStream_t)stream, x, mean, std_out, S, Q);
    IDIFF_CHECK_LAUNCH("ensemble_stats");
    return IDIFF_OK;
}

// ---- posterior ensembles: per-pixel order statistics and interval coverage ----
namespace {

constexpr int ORD_MAX_K = 8;     // output planes per launch
constexpr int ORD_NET_MAX = 16;  // the network form keeps a thread's S float4 in registers up to here (= ENS_REG)
struct OrderKs {
    int k[ORD_MAX_K];
};

// Batcher's odd-even merge sort on n = 2^m wires as a fixed list of compare-exchanges (a, b), a < b, evaluated at compile time:
// comparator idx of the list, or {-1, idx's excess over the list} past its end.  n = 2, 4, 8, 16 -> 1, 5, 19, 63 comparators.
struct CePair {
    int a, b;
};
constexpr CePair oem_pair(int n, int idx) {
    int seen = 0;
    for (int p = 1; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < n; j += 2 * k)
                for (int i = 0; i < k && i + j + k < n; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        if (seen == idx) return CePair{i + j, i + j + k};
                        ++seen;
                    }
    return CePair{-1, seen};
}
constexpr int oem_count(int n) { return oem_pair(n, 1 << 30).b; }
static_assert(oem_count(1) == 0 && oem_count(2) == 1 && oem_count(4) == 5 && oem_count(8) == 19 && oem_count(16) == 63, "odd-even merge sort");

// v_min_f32 / v_max_f32 per lane: both return one of their operands' values, so the network permutes values and rounds nothing
template <int NP, int I>
__device__ __forceinline__ void oem_exchange(floatx4 (&val)[NP]) {
    constexpr int a = oem_pair(NP, I).a, b = oem_pair(NP, I).b;
    static_assert(a >= 0 && a < b && b < NP, "comparator out of range");
    const floatx4 lo = val[a], hi = val[b];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        val[a][e] = fminf(lo[e], hi[e]);
        val[b][e] = fmaxf(lo[e], hi[e]);
    }
}
template <int NP, int... I>
__device__ __forceinline__ void oem_sort(floatx4 (&val)[NP], std::integer_sequence<int, I...>) {
    (oem_exchange<NP, I>(val), ...);
}

// val[k] for a wave-uniform k in [0, NP): a uniform branch to one constant-index read, so val[] is never indexed at run time (no
// scratch) and the choice costs no per-lane select
template <int NP>
__device__ __forceinline__ floatx4 order_pick(const floatx4 (&val)[NP], int k) {
    floatx4 o = val[0];
#define ORD_CASE(s)                       \
    case s:                               \
        if constexpr (s < NP) o = val[s]; \
        break;
    switch (k) {
        ORD_CASE(1) ORD_CASE(2) ORD_CASE(3) ORD_CASE(4) ORD_CASE(5) ORD_CASE(6) ORD_CASE(7) ORD_CASE(8)
        ORD_CASE(9) ORD_CASE(10) ORD_CASE(11) ORD_CASE(12) ORD_CASE(13) ORD_CASE(14) ORD_CASE(15)
        default:
            break;
    }
#undef ORD_CASE
    return o;
}
static_assert(ORD_NET_MAX == 16, "order_pick lists 16 cases");

// Network form, S <= NP <= 16: a thread loads its S float4 into registers (padded with +inf to NP), sorts them ascending through the
// fixed network and stores registers ks[0..nk), each picked by order_pick, so val[] stays in VGPRs.  A NaN among the S values of a pixel makes every plane NaN there.
template <int NP>
__global__ __launch_bounds__(256) void ensemble_order_net_kernel(const float* __restrict__ x, float* __restrict__ out, int S, int nk, long long Q,
                                                                 OrderKs ks) {
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    floatx4* os = reinterpret_cast<floatx4*>(out) + (long long)blockIdx.y * nk * Q;
    const float inf = __builtin_huge_valf(), qnan = __builtin_nanf("");
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        floatx4 val[NP];
        bool bad[4] = {false, false, false, false};
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            if (s < S) {
                val[s] = xs[(long long)s * Q + v];
#pragma unroll
                for (int e = 0; e < 4; ++e) bad[e] |= val[s][e] != val[s][e];
            } else {
                val[s] = floatx4{inf, inf, inf, inf};
            }
        }
        oem_sort<NP>(val, std::make_integer_sequence<int, oem_count(NP)>{});
#pragma unroll
        for (int i = 0; i < ORD_MAX_K; ++i)
            if (i < nk) {
                floatx4 o = order_pick<NP>(val, ks.k[i]);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = bad[e] ? qnan : o[e];
                os[(long long)i * Q + v] = o;
            }
    }
}

// Rank form, any S: candidate s has rank #{j : x_j < x_s} + #{j < s : x_j == x_s}, a permutation of 0..S-1 when no value is NaN, and the
// candidate of rank ks[i] is plane i's value.  Candidates are taken ORD_CH at a time in registers, so the S values are read S / ORD_CH
// times (the re-reads hit L2); members before the chunk count with <=, members after it with <, members inside it by their index.  The
// nk outputs collect in registers and are stored once per pixel, with the network form's NaN rule.
constexpr int ORD_CH = 4;
__global__ __launch_bounds__(256) void ensemble_order_rank_kernel(const float* __restrict__ x, float* __restrict__ out, int S, int nk, long long Q,
                                                                  OrderKs ks) {
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    floatx4* os = reinterpret_cast<floatx4*>(out) + (long long)blockIdx.y * nk * Q;
    const float qnan = __builtin_nanf("");
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        floatx4 o[ORD_MAX_K];
        bool bad[4] = {false, false, false, false};
#pragma unroll
        for (int i = 0; i < ORD_MAX_K; ++i) o[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < S; s0 += ORD_CH) {
            floatx4 cand[ORD_CH];
            int rank[ORD_CH][4];
#pragma unroll
            for (int c = 0; c < ORD_CH; ++c) {
                const int s = s0 + c < S ? s0 + c : S - 1;  // past the end: a copy of the last member, never selected
                cand[c] = xs[(long long)s * Q + v];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bad[e] |= cand[c][e] != cand[c][e];
                    rank[c][e] = 0;
                }
            }
            for (int j = 0; j < s0; ++j) {
                const floatx4 xj = xs[(long long)j * Q + v];
#pragma unroll
                for (int c = 0; c < ORD_CH; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) rank[c][e] += xj[e] <= cand[c][e] ? 1 : 0;
            }
#pragma unroll
            for (int jj = 0; jj < ORD_CH; ++jj)
                if (s0 + jj < S) {
#pragma unroll
                    for (int c = 0; c < ORD_CH; ++c) {
                        if (c == jj) continue;
#pragma unroll
                        for (int e = 0; e < 4; ++e) rank[c][e] += (jj < c ? cand[jj][e] <= cand[c][e] : cand[jj][e] < cand[c][e]) ? 1 : 0;
                    }
                }
            for (int j = s0 + ORD_CH; j < S; ++j) {
                const floatx4 xj = xs[(long long)j * Q + v];
#pragma unroll
                for (int c = 0; c < ORD_CH; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) rank[c][e] += xj[e] < cand[c][e] ? 1 : 0;
            }
#pragma unroll
            for (int c = 0; c < ORD_CH; ++c)
                if (s0 + c < S) {
#pragma unroll
                    for (int i = 0; i < ORD_MAX_K; ++i)
                        if (i < nk) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) o[i][e] = rank[c][e] == ks.k[i] ? cand[c][e] : o[i][e];
                        }
                }
        }
#pragma unroll
        for (int i = 0; i < ORD_MAX_K; ++i)
            if (i < nk) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[i][e] = bad[e] ? qnan : o[i][e];
                os[(long long)i * Q + v] = o[i];
            }
    }
}

// Interval coverage: integer counts {target < lo, lo <= target <= hi, target > hi} per image; a pixel where any of the three is NaN
// counts nowhere.  COV_PARTS blocks per image write partial counts, a second launch adds them: integers only, no atomics.
constexpr int COV_PARTS = 64;
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(256) void interval_coverage_partial_kernel(const float* __restrict__ lo, const float* __restrict__ hi,
                                                                        const float* __restrict__ tgt, int32_t* __restrict__ part, long long Q) {
    __shared__ int red[3][4];
    const long long row = (long long)blockIdx.y * Q;
    const floatx4* l4 = reinterpret_cast<const floatx4*>(lo) + row;
    const floatx4* h4 = reinterpret_cast<const floatx4*>(hi) + row;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + row;
    int below = 0, inside = 0, above = 0;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        const floatx4 lv = l4[v], hv = h4[v], tv = t4[v];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = lv[e] == lv[e] && hv[e] == hv[e];  // a NaN target fails every comparison below by itself
            below += (ok && tv[e] < lv[e]) ? 1 : 0;
            inside += (ok && tv[e] >= lv[e] && tv[e] <= hv[e]) ? 1 : 0;
            above += (ok && tv[e] > hv[e]) ? 1 : 0;
        }
    }
    below = wave_sum_int(below);
    inside = wave_sum_int(inside);
    above = wave_sum_int(above);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = below;
        red[1][threadIdx.x >> 6] = inside;
        red[2][threadIdx.x >> 6] = above;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        part[((long long)blockIdx.y * COV_PARTS + blockIdx.x) * 3 + threadIdx.x] =
            (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ void interval_coverage_final_kernel(const int32_t* __restrict__ part, int32_t* __restrict__ counts, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (b, which)
    if (i >= B * 3) return;
    const int b = i / 3, w = i - b * 3;
    int acc = 0;
    for (int p = 0; p < COV_PARTS; ++p) acc += part[((long long)b * COV_PARTS + p) * 3 + w];
    counts[i] = acc;
}

template <int NP>
void launch_order_net(const float* x, float* out, int B, int S, int nk, long long Q, const OrderKs& ks, hipStream_t st) {
    hipLaunchKernelGGL(ensemble_order_net_kernel<NP>, rows_grid(Q, B), dim3(256), 0, st, x, out, S, nk, Q, ks);
}

}  // namespace

extern "C" int idiff_ensemble_order_stats(const float* x, float* out, int B, int S, int64_t n_s, const int32_t* ks_host, int nk, int algo,
                                          idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && out && ks_host && B > 0 && B <= 65535 && S > 0 && n_s > 0, "ensemble_order_stats: bad args");
    IDIFF_CHECK_ARG(nk >= 1 && nk <= ORD_MAX_K, "ensemble_order_stats: nk = %d is outside [1, %d]", nk, ORD_MAX_K);
    IDIFF_CHECK_ARG(algo >= 0 && algo <= 2, "ensemble_order_stats: algo must be 0 (auto), 1 (network) or 2 (rank), got %d", algo);
    IDIFF_CHECK_ARG(algo != 1 || S <= ORD_NET_MAX, "ensemble_order_stats: the network form holds at most %d members, got S = %d", ORD_NET_MAX, S);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_order_stats: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({x, out}), "ensemble_order_stats: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(out != x, "ensemble_order_stats: out must not be x");
    OrderKs ks;
    for (int i = 0; i < ORD_MAX_K; ++i) {
        ks.k[i] = i < nk ? ks_host[i] : 0;
        IDIFF_CHECK_ARG(ks.k[i] >= 0 && ks.k[i] < S, "ensemble_order_stats: ks[%d] = %d is outside [0, S = %d)", i, ks.k[i], S);
    }
    const long long Q = n_s / 4;
    hipStream_t st = (hipStream_t)stream;
    if (algo == 2 || S > ORD_NET_MAX)
        hipLaunchKernelGGL(ensemble_order_rank_kernel, rows_grid(Q, B), dim3(256), 0, st, x, out, S, nk, Q, ks);
    else if (S == 1)
        launch_order_net<1>(x, out, B, S, nk, Q, ks, st);
    else if (S == 2)
        launch_order_net<2>(x, out, B, S, nk, Q, ks, st);
    else if (S <= 4)
        launch_order_net<4>(x, out, B, S, nk, Q, ks, st);
    else if (S <= 8)
        launch_order_net<8>(x, out, B, S, nk, Q, ks, st);
    else
        launch_order_net<16>(x, out, B, S, nk, Q, ks, st);
    IDIFF_CHECK_LAUNCH("ensemble_order_stats");
    return IDIFF_OK;
}

extern "C" int64_t idiff_interval_coverage_ws_ints(int B, int64_t n_s) {
    (void)n_s;
    return B > 0 ? (int64_t)B * COV_PARTS * 3 : 0;
}

extern "C" int idiff_interval_coverage(const float* lo, const float* hi, const float* target, int32_t* counts, int32_t* ws, int B, int64_t n_s,
                                       idiff_stream_t stream) {
    IDIFF_CHECK_ARG(lo && hi && target && counts && ws && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL, "interval_coverage: bad args");
    IDIFF_CHECK_ARG(n_s % 4 == 0, "interval_coverage: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({lo, hi, target}), "interval_coverage: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG(counts != ws, "interval_coverage: counts must not be ws");
    const long long Q = n_s / 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(interval_coverage_partial_kernel, dim3(COV_PARTS, (unsigned)B), dim3(256), 0, st, lo, hi, target, ws, Q);
    IDIFF_CHECK_LAUNCH("interval_coverage_partial");
    hipLaunchKernelGGL(interval_coverage_final_kernel, dim3((B * 3 + 63) / 64), dim3(64), 0, st, (const int32_t*)ws, counts, B);
    IDIFF_CHECK_LAUNCH("interval_coverage_final");
    return IDIFF_OK;
}

// ---- posterior ensembles: CRPS, rank histogram and spread-skill sums (the contract is in include/idiff.h) ----
namespace {

constexpr int SCORE_PARTS = 64;    // partial blocks per image (= COV_PARTS)
constexpr int SCORE_MAX_S = 1024;  // the block's LDS histogram holds S + 2 <= 1026 bins
constexpr int SCORE_CH = 4;        // candidates per chunk of the second-read form (= ORD_CH)
constexpr int SCORE_REG = 16;      // the register form's largest S (= ENS_REG); the dispatch lists its 16 cases

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What a thread carries through its grid-stride loop: the fp64 sums of its valid pixels' fp32 crps, e, v, in loop order.
struct ScoreAcc {
    double crps = 0.0, e = 0.0, v = 0.0;
};

// The end of a pixel: a, g, ss as in the contract, e = m*m already formed by the caller.  The quotients are IEEE fp32 divisions (S, S^2 <=
// 2^20 and S - 1 are exact floats), correctly rounded like the fp64 route of ensemble_stats_kernel.  Invalid (a NaN d_s): NaN in the
// map, bin S + 1, nothing added.  k <= S by construction, so the LDS index stays inside hist[S + 2] whatever the data.
__device__ __forceinline__ float score_pixel(float a, float g, float ss, float ev, int k, bool bad, int S, ScoreAcc& acc, int* hist) {
    const float crps = __fsub_rn(__fdiv_rn(a, (float)S), __fdiv_rn(g, (float)(S * S)));
    const float var = S > 1 ? __fdiv_rn(ss, (float)(S - 1)) : 0.f;
    atomicAdd(&hist[bad ? S + 1 : k], 1);  // integer LDS add: order-independent
    if (bad) return __builtin_nanf("");
    acc.crps += (double)crps;
    acc.e += (double)ev;
    acc.v += (double)var;
    return crps;
}

__device__ __forceinline__ void score_block_begin(int* hist, int S) {
    for (int i = threadIdx.x; i < S + 2; i += blockDim.x) hist[i] = 0;
    __syncthreads();
}

// Wave tree, then the four waves in index order; one fp64 partial per quantity and block, and the block's histogram beside it.
__device__ __forceinline__ void score_block_end(const ScoreAcc& acc, const int* hist, double (&red)[3][4], double* __restrict__ part_sums,
                                                int32_t* __restrict__ part_hist, int S) {
    const double c = wave_sum_f64(acc.crps), e = wave_sum_f64(acc.e), v = wave_sum_f64(acc.v);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = c;
        red[1][threadIdx.x >> 6] = e;
        red[2][threadIdx.x >> 6] = v;
    }
    __syncthreads();  // also: every LDS add of the block has landed
    const long long blk = (long long)blockIdx.y * SCORE_PARTS + blockIdx.x;
    if (threadIdx.x < 3) part_sums[blk * 3 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
    for (int i = threadIdx.x; i < S + 2; i += blockDim.x) part_hist[blk * (S + 2) + i] = hist[i];
}

// Register form, S <= 16, one instantiation per S: a thread's S float4 of d_s = x_s - y stay in registers (constant indices only), and
// the S rank counters of one element at a time.  Each unordered pair (j < s) is compared once: le = d_j <= d_s puts j below s, !le puts s
// below j (no NaN on a valid pixel), so rank_s = (S - 1 - s) + sum_{j < s} le(j, s) - sum_{t > s} le(s, t): S (S - 1)/2 compares per
// element, each a v_cmp and two add / subtract-with-carry.  Up to S = 12 the kernel is held to 128 VGPRs, so that four waves per SIMD
// -- the 64-block grids of 16 images at once -- are resident; S = 16 takes 147 (three waves); no instantiation uses scratch.
template <int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S <= 12 ? 4 : 3))) void ensemble_scores_reg_kernel(
    const float* __restrict__ x, const float* __restrict__ tgt, float* __restrict__ map, double* __restrict__ part_sums,
    int32_t* __restrict__ part_hist, long long Q) {
    __shared__ int hist[SCORE_MAX_S + 2];
    __shared__ double red[3][4];
    score_block_begin(hist, S);
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + (long long)blockIdx.y * Q;
    floatx4* m4 = map ? reinterpret_cast<floatx4*>(map) + (long long)blockIdx.y * Q : nullptr;
    ScoreAcc acc;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        const floatx4 y = t4[v];
        floatx4 d[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const floatx4 xv = xs[(long long)s * Q + v];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[s][e] = __fsub_rn(xv[e], y[e]);
        }
        floatx4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = 0.f, g = 0.f, sd = 0.f, ss = 0.f;
            int k = 0;
            bool bad = false;
            int rank[S];  // one compare per unordered pair: le puts j below s, !le puts s below j (no NaN on a valid pixel)
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
            o[e] = score_pixel(a, g, ss, __fmul_rn(m, m), k, bad, S, acc, hist);
        }
        if (m4) m4[v] = o;
    }
    score_block_end(acc, hist, red, part_sums, part_hist, S);
}

// Second-read form, any S: one pass over the members for a, the mean and k, then candidates SCORE_CH at a time in index order, each
// chunk walking all S members again for its ranks (ensemble_order_rank_kernel's compares, on d instead of x; the re-reads hit L2).  g and
// the squared deviations are added as the chunks finish, i.e. in member order: the same operations in the same order as the register form.
__global__ __launch_bounds__(256) void ensemble_scores_reread_kernel(const float* __restrict__ x, const float* __restrict__ tgt, float* __restrict__ map,
                                                                     double* __restrict__ part_sums, int32_t* __restrict__ part_hist, int S, long long Q) {
    __shared__ int hist[SCORE_MAX_S + 2];
    __shared__ double red[3][4];
    score_block_begin(hist, S);
    const floatx4* xs = reinterpret_cast<const floatx4*>(x) + (long long)blockIdx.y * S * Q;
    const floatx4* t4 = reinterpret_cast<const floatx4*>(tgt) + (long long)blockIdx.y * Q;
    floatx4* m4 = map ? reinterpret_cast<floatx4*>(map) + (long long)blockIdx.y * Q : nullptr;
    ScoreAcc acc;
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < Q; v += (long long)gridDim.x * blockDim.x) {
        const floatx4 y = t4[v];
        floatx4 a = {0.f, 0.f, 0.f, 0.f}, g = a, sd = a, ss = a, mv, ev;
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
        for (int e = 0; e < 4; ++e) {
            mv[e] = __fdiv_rn(sd[e], (float)S);
            ev[e] = __fmul_rn(mv[e], mv[e]);
        }
        for (int s0 = 0; s0 < S; s0 += SCORE_CH) {
            floatx4 cand[SCORE_CH];
            int rank[SCORE_CH][4];
#pragma unroll
            for (int c = 0; c < SCORE_CH; ++c) {
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
                    for (int c = 0; c < SCORE_CH; ++c) rank[c][e] += dj <= cand[c][e] ? 1 : 0;
                }
            }
#pragma unroll
            for (int jj = 0; jj < SCORE_CH; ++jj)
                if (s0 + jj < S) {
#pragma unroll
                    for (int c = 0; c < SCORE_CH; ++c) {
                        if (c == jj) continue;
#pragma unroll
                        for (int e = 0; e < 4; ++e) rank[c][e] += (jj < c ? cand[jj][e] <= cand[c][e] : cand[jj][e] < cand[c][e]) ? 1 : 0;
                    }
                }
            for (int j = s0 + SCORE_CH; j < S; ++j) {
                const floatx4 xj = xs[(long long)j * Q + v];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dj = __fsub_rn(xj[e], y[e]);
#pragma unroll
                    for (int c = 0; c < SCORE_CH; ++c) rank[c][e] += dj < cand[c][e] ? 1 : 0;
                }
            }
#pragma unroll
            for (int c = 0; c < SCORE_CH; ++c)
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
        floatx4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = score_pixel(a[e], g[e], ss[e], ev[e], k[e], bad[e], S, acc, hist);
        if (m4) m4[v] = o;
    }
    score_block_end(acc, hist, red, part_sums, part_hist, S);
}

// One block per image.  The 3 x SCORE_PARTS fp64 partials are fetched by as many threads at once and added from LDS in index order by
// one thread per quantity; a bin's integer partials are fetched eight at a time (integer addition: any order gives the same count).
__global__ __launch_bounds__(256) void ensemble_scores_final_kernel(const double* __restrict__ part_sums, const int32_t* __restrict__ part_hist,
                                                                    double* __restrict__ sums, int32_t* __restrict__ counts, int S) {
    __shared__ double part[3][SCORE_PARTS];
    const long long b = blockIdx.x;
    if (threadIdx.x < 3 * SCORE_PARTS) {
        const int q = threadIdx.x / SCORE_PARTS, p = threadIdx.x % SCORE_PARTS;
        part[q][p] = part_sums[(b * SCORE_PARTS + p) * 3 + q];
    }
    for (int i = threadIdx.x; i < S + 2; i += blockDim.x) {
        const int32_t* col = part_hist + b * SCORE_PARTS * (S + 2) + i;
        int acc = 0;
#pragma unroll 8
        for (int p = 0; p < SCORE_PARTS; ++p) acc += col[(long long)p * (S + 2)];
        counts[b * (S + 2) + i] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = part[threadIdx.x][0];
        for (int p = 1; p < SCORE_PARTS; ++p) acc += part[threadIdx.x][p];
        sums[b * 3 + threadIdx.x] = acc;
    }
}

template <int S>
void launch_scores_reg(const float* x, const float* tgt, float* map, double* ps, int32_t* ph, int B, long long Q, hipStream_t st) {
    hipLaunchKernelGGL(ensemble_scores_reg_kernel<S>, dim3(SCORE_PARTS, (unsigned)B), dim3(256), 0, st, x, tgt, map, ps, ph, Q);
}

}  // namespace

extern "C" int64_t idiff_ensemble_scores_ws_bytes(int B, int S) {
    if (B <= 0 || B > 65535 || S <= 0 || S > SCORE_MAX_S) return 0;
    return (int64_t)B * SCORE_PARTS * (3 * (int64_t)sizeof(double) + (S + 2) * (int64_t)sizeof(int32_t));
}

extern "C" int idiff_ensemble_scores(const float* x, const float* target, float* crps_map, double* sums, int32_t* counts, void* ws, int B, int S,
                                     int64_t n_s, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(x && target && sums && counts && ws && B > 0 && B <= 65535 && n_s > 0 && n_s <= 0x7fffffffLL, "ensemble_scores: bad args");
    IDIFF_CHECK_ARG(S >= 1 && S <= SCORE_MAX_S, "ensemble_scores: S = %d is outside [1, %d]", S, SCORE_MAX_S);
    IDIFF_CHECK_ARG(n_s % 4 == 0, "ensemble_scores: n_s = %lld is not a multiple of 4", (long long)n_s);
    IDIFF_CHECK_ARG(aligned16({x, target, crps_map}), "ensemble_scores: operands must be 16-byte aligned");
    IDIFF_CHECK_ARG((uintptr_t)sums % 8 == 0 && (uintptr_t)ws % 8 == 0 && (uintptr_t)counts % 4 == 0,
                    "ensemble_scores: sums and ws must be 8-byte aligned, counts 4-byte aligned");
    IDIFF_CHECK_ARG(crps_map != x && crps_map != target, "ensemble_scores: crps_map must not be x or target");
    IDIFF_CHECK_ARG(ws != (void*)sums && ws != (void*)counts && (void*)sums != (void*)counts && ws != (void*)x && ws != (void*)target &&
                        ws != (void*)crps_map,
                    "ensemble_scores: ws, sums and counts must be buffers of their own");
    const long long Q = n_s / 4;
    hipStream_t st = (hipStream_t)stream;
    double* ps = static_cast<double*>(ws);
    int32_t* ph = reinterpret_cast<int32_t*>(ps + (long long)B * SCORE_PARTS * 3);
    // IDIFF_ENSEMBLE_REREAD=1 (tests): the second-read form also where the values would fit in registers, as in idiff_ensemble_stats
    const char* rr = getenv("IDIFF_ENSEMBLE_REREAD");
    if (S > SCORE_REG || (rr && rr[0] == '1')) {
        hipLaunchKernelGGL(ensemble_scores_reread_kernel, dim3(SCORE_PARTS, (unsigned)B), dim3(256), 0, st, x, target, crps_map, ps, ph, S, Q);
    } else {
#define SCORE_CASE(s)                                                   \
    case s:                                                             \
        launch_scores_reg<s>(x, target, crps_map, ps, ph, B, Q, st); \
        break;
        switch (S) {
            SCORE_CASE(1) SCORE_CASE(2) SCORE_CASE(3) SCORE_CASE(4) SCORE_CASE(5) SCORE_CASE(6) SCORE_CASE(7) SCORE_CASE(8)
            SCORE_CASE(9) SCORE_CASE(10) SCORE_CASE(11) SCORE_CASE(12) SCORE_CASE(13) SCORE_CASE(14) SCORE_CASE(15) SCORE_CASE(16)
        }
#undef SCORE_CASE
    }
    IDIFF_CHECK_LAUNCH("ensemble_scores_partial");
    hipLaunchKernelGGL(ensemble_scores_final_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)ps, (const int32_t*)ph, sums, counts, S);
    IDIFF_CHECK_LAUNCH("ensemble_scores_final");
    return IDIFF_OK;
}
