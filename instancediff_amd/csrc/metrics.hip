// On-device validation metrics of the drivers (trainUM.py:314-329, testUM.py:151-164): RMSE / PSNR (data_range 1)
// and SSIM with skimage's settings (gaussian_weights=True, sigma=1.5 -> 11x11 window, use_sample_covariance=False,
// K1=.01, K2=.03, data_range=1, mean over the interior cropped by (win-1)/2) on images mapped x/2+0.5.
// Replaces a per-image device->host copy + skimage call by one launch per batch and one [B,3] read-back.
//
// Operation order (fp32 unless said; tests/image_metrics_ref.py restates it).  Per interior pixel the five window moments are taken on
// values shifted by the window-centre pixels, da = 0.5 (p - p0), dc = 0.5 (t - t0):  sx = sum w da, sy = sum w dc, sxx = sum w da^2,
// syy = sum w dc^2, sxy = sum w da dc over the 11x11 window, row by row;  vx = sxx - sx^2, vy = syy - sy^2, vxy = sxy - sx sy (variances
// and the covariance do not see a shift) and the means get the shifts back, ux = (0.5 p0 + 0.5) + sx, uy = (0.5 t0 + 0.5) + sy.  Raw
// moments sum w a^2 - (sum w a)^2 lose a^2 2^-24 sqrt(121) to rounding, against C2 = 9e-4 in the denominator: up to 6e-4 of SSIM on a
// locally flat bright image, which is what clamped CT and cryo-EM data are made of.  The quotient is evaluated without FMA contraction,
// so that its numerator and denominator are the same roundings of the same numbers when pred == target (SSIM exactly 1).
// Reduction: thread i of 64 x 256 adds the values of pixels i, i + 16384, ...; a 64-lane xor butterfly; the workgroup's four waves as
// (w0 + w1) + (w2 + w3); metrics_final_kernel sums the 64 partials of an image in fp64, in order.
// H < 11 or W < 11: no pixel has a whole window and SSIM is NaN (skimage refuses such an image), not 0.
#include <math.h>

#include "common.h"

namespace {

constexpr int SS_R = 5;  // radius: int(3.5 * 1.5 + 0.5)
constexpr int SS_PARTS = 64;

__device__ __forceinline__ float ssim_index(float ux, float uy, float vx, float vy, float vxy) {
#pragma clang fp contract(off)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    return ((2.f * ux * uy + C1) * (2.f * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
}

__global__ __launch_bounds__(256) void metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, float* __restrict__ part,
                                                              int H, int W) {
    __shared__ float w1[2 * SS_R + 1];
    __shared__ float red[2][4];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = -SS_R; i <= SS_R; ++i) {
            w1[i + SS_R] = expf(-0.5f * (float)(i * i) / (1.5f * 1.5f));
            s += w1[i + SS_R];
        }
        for (int i = 0; i <= 2 * SS_R; ++i) w1[i] /= s;
    }
    __syncthreads();
    const float* p = pred + (long long)b * H * W;
    const float* t = tgt + (long long)b * H * W;
    float sse = 0.f, ssim = 0.f;
    const int n = H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / W, x = i - y * W;
        const float d = 0.5f * (p[i] - t[i]);  // (p/2+0.5) - (t/2+0.5)
        sse += d * d;
        if (y >= SS_R && y < H - SS_R && x >= SS_R && x < W - SS_R) {
            const float p0 = p[i], t0 = t[i];
            float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
            for (int dy = -SS_R; dy <= SS_R; ++dy) {
                const float wy = w1[dy + SS_R];
                for (int dx = -SS_R; dx <= SS_R; ++dx) {
                    const float w = wy * w1[dx + SS_R];
                    const float a = 0.5f * (p[(y + dy) * W + x + dx] - p0);
                    const float c = 0.5f * (t[(y + dy) * W + x + dx] - t0);
                    sx += w * a;
                    sy += w * c;
                    sxx += w * a * a;
                    syy += w * c * c;
                    sxy += w * a * c;
                }
            }
            const float vx = sxx - sx * sx, vy = syy - sy * sy, vxy = sxy - sx * sy;
            ssim += ssim_index((0.5f * p0 + 0.5f) + sx, (0.5f * t0 + 0.5f) + sy, vx, vy, vxy);
        }
    }
    sse = wave_sum(sse);
    ssim = wave_sum(ssim);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sse;
        red[1][threadIdx.x >> 6] = ssim;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[((long long)b * SS_PARTS + blockIdx.x) * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        part[((long long)b * SS_PARTS + blockIdx.x) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ void metrics_final_kernel(const float* __restrict__ part, float* __restrict__ out, int B, int H, int W) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sse = 0.0, ss = 0.0;
    for (int i = 0; i < SS_PARTS; ++i) {
        sse += (double)part[((long long)b * SS_PARTS + i) * 2];
        ss += (double)part[((long long)b * SS_PARTS + i) * 2 + 1];
    }
    const double mse = sse / ((double)H * W);
    const double inner = (double)(H - 2 * SS_R) * (double)(W - 2 * SS_R);
    out[b * 3 + 0] = (float)sqrt(mse);
    out[b * 3 + 1] = (float)(10.0 * log10(1.0 / mse));
    out[b * 3 + 2] = (H > 2 * SS_R && W > 2 * SS_R) ? (float)(ss / inner) : nanf("");
}

}  // namespace

extern "C" int idiff_image_metrics(const float* pred, const float* target, float* out_b3, float* ws, int B, int H, int W, idiff_stream_t stream) {
    IDIFF_CHECK_ARG(pred && target && out_b3 && ws && B > 0 && H > 0 && W > 0, "image_metrics: bad args");
    hipLaunchKernelGGL(metrics_partial_kernel, dim3(SS_PARTS, B), dim3(256), 0, (hipStream_t)stream, pred, target, ws, H, W);
    IDIFF_CHECK_LAUNCH("image_metrics_partial");
    hipLaunchKernelGGL(metrics_final_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, ws, out_b3, B, H, W);
    IDIFF_CHECK_LAUNCH("image_metrics_final");
    return IDIFF_OK;
}
