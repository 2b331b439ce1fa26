// Image-quality metrics of the evaluation step that follows the rollout (reference lib/metrics.py:
// PSNR :181-212, SSIM :216-255, both delegating to piqa==1.2.2), fused with the evaluator's clamp
// (05_evaluate_predictor.py:96-99) so predicted frames are read once.
//
//   PSNR_n = 10 log10(1 / (mean_{c,h,w} (x-y)^2 + 1e-8))                       (piqa.psnr, value_range 1)
//   SSIM_n = mean_{c,h',w'} [(2 mu_x mu_y + c1)(2 s_xy + c2)] / [(mu_x^2 + mu_y^2 + c1)(s_xx + s_yy + c2)]
//            with an 11-tap Gaussian (sigma 1.5) window applied separably per channel, VALID padding,
//            c1 = 0.01^2, c2 = 0.03^2, s_ab = E[ab] - mu_a mu_b                  (piqa.ssim.SSIM defaults)
//
// One workgroup per (image, channel): both planes are clamped into LDS once, every thread evaluates
// the 11x11 window for its output pixels from LDS (tiny problem: 3.2 GFLOP for a 608-frame batch),
// partial sums go to a workspace and a second kernel reduces them in a fixed order (deterministic).
// Frames whose two planes do not fit in LDS (H*W*8 > 160 KiB - 64, above about 143x143: the ExtendedDINOSAUR family at
// 224 / 336) take the banded form: one workgroup per (image, channel, band of output rows) stages its band plus the
// 10-row halo of both planes, per-band partial sums are reduced in a fixed order.  Frames that fit keep the one-workgroup
// form bit for bit.  H, W >= 11 (valid SSIM window).
#include "common.h"

namespace {

constexpr int WIN = 11;

__global__ __launch_bounds__(256) void metric_partial_kernel(const float* __restrict__ preds,
                                                             const float* __restrict__ targets,
                                                             float* __restrict__ ws, int C, int H,
                                                             int W, int do_clamp) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xs = sm;
    float* ys = sm + H * W;
    __shared__ float red[2][4];
    const int t = threadIdx.x, c = blockIdx.x, n = blockIdx.y;
    const float* xp = preds + ((size_t)n * C + c) * H * W;
    const float* yp = targets + ((size_t)n * C + c) * H * W;

    float g[WIN];
    {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            const float d = (float)i - 0.5f * (WIN - 1);
            g[i] = expf(-d * d / (2.f * 1.5f * 1.5f));
            s += g[i];
        }
#pragma unroll
        for (int i = 0; i < WIN; ++i) g[i] /= s;
    }

    float sq = 0.f;
    for (int i = t; i < H * W; i += 256) {
        float x = xp[i], y = yp[i];
        if (do_clamp) {
            x = fminf(fmaxf(x, 0.f), 1.f);
            y = fminf(fmaxf(y, 0.f), 1.f);
        }
        xs[i] = x;
        ys[i] = y;
        sq += (x - y) * (x - y);
    }
    __syncthreads();

    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float ss = 0.f;
    for (int o = t; o < OH * OW; o += 256) {
        const int oy = o / OW, ox = o % OW;
        float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
        for (int i = 0; i < WIN; ++i) {
            float rx = 0.f, ry = 0.f, rxx = 0.f, ryy = 0.f, rxy = 0.f;
            const float* xr = xs + (oy + i) * W + ox;
            const float* yr = ys + (oy + i) * W + ox;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const float x = xr[j], y = yr[j], w = g[j];
                rx = fmaf(w, x, rx);
                ry = fmaf(w, y, ry);
                rxx = fmaf(w, x * x, rxx);
                ryy = fmaf(w, y * y, ryy);
                rxy = fmaf(w, x * y, rxy);
            }
            mx = fmaf(g[i], rx, mx);
            my = fmaf(g[i], ry, my);
            mxx = fmaf(g[i], rxx, mxx);
            myy = fmaf(g[i], ryy, myy);
            mxy = fmaf(g[i], rxy, mxy);
        }
        const float sxx = mxx - mx * mx, syy = myy - my * my, sxy = mxy - mx * my;
        const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
        ss += (2.f * mx * my + c1) / (mx * mx + my * my + c1) * cs;
    }

    sq = wave_sum64(sq);
    ss = wave_sum64(ss);
    if ((t & 63) == 0) {
        red[0][t >> 6] = sq;
        red[1][t >> 6] = ss;
    }
    __syncthreads();
    if (t == 0) {
        ws[((size_t)n * C + c) * 2 + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        ws[((size_t)n * C + c) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void metric_final_kernel(const float* __restrict__ ws,
                                                           float* __restrict__ psnr,
                                                           float* __restrict__ ssim, int N, int C,
                                                           int H, int W) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float sq = 0.f, ss = 0.f;
    for (int c = 0; c < C; ++c) {
        sq += ws[((size_t)n * C + c) * 2 + 0];
        ss += ws[((size_t)n * C + c) * 2 + 1];
    }
    const float mse = sq / (float)(C * H * W);
    if (psnr) psnr[n] = 10.f * log10f(1.f / (mse + 1e-8f));
    if (ssim) ssim[n] = ss / (float)(C * (H - WIN + 1) * (W - WIN + 1));
}

// Banded form: grid (band, channel, image).  Band b covers output rows [b BR, min((b + 1) BR, OH)) and stages input rows
// [b BR, that + 10); its squared errors are those of input rows [b BR, (b + 1) BR), the last band also takes the final 10.
__global__ __launch_bounds__(256) void metric_band_kernel(const float* __restrict__ preds,
                                                          const float* __restrict__ targets,
                                                          float* __restrict__ ws, int C, int H, int W, int BR,
                                                          int do_clamp) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[2][4];
    const int t = threadIdx.x, b = blockIdx.x, c = blockIdx.y, n = blockIdx.z, nb = gridDim.x;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const int r0 = b * BR, r1 = min(r0 + BR, OH), rows = r1 - r0 + WIN - 1;
    const int sq_end = (b == nb - 1 ? H : r1) - r0;
    float* xs = sm;
    float* ys = sm + (size_t)rows * W;
    const float* xp = preds + ((size_t)n * C + c) * H * W + (size_t)r0 * W;
    const float* yp = targets + ((size_t)n * C + c) * H * W + (size_t)r0 * W;

    float g[WIN];
    {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            const float d = (float)i - 0.5f * (WIN - 1);
            g[i] = expf(-d * d / (2.f * 1.5f * 1.5f));
            s += g[i];
        }
#pragma unroll
        for (int i = 0; i < WIN; ++i) g[i] /= s;
    }

    float sq = 0.f;
    for (int i = t; i < rows * W; i += 256) {
        float x = xp[i], y = yp[i];
        if (do_clamp) {
            x = fminf(fmaxf(x, 0.f), 1.f);
            y = fminf(fmaxf(y, 0.f), 1.f);
        }
        xs[i] = x;
        ys[i] = y;
        if (i < sq_end * W) sq += (x - y) * (x - y);
    }
    __syncthreads();

    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float ss = 0.f;
    for (int o = t; o < (r1 - r0) * OW; o += 256) {
        const int oy = o / OW, ox = o % OW;
        float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
        for (int i = 0; i < WIN; ++i) {
            float rx = 0.f, ry = 0.f, rxx = 0.f, ryy = 0.f, rxy = 0.f;
            const float* xr = xs + (oy + i) * W + ox;
            const float* yr = ys + (oy + i) * W + ox;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const float x = xr[j], y = yr[j], w = g[j];
                rx = fmaf(w, x, rx);
                ry = fmaf(w, y, ry);
                rxx = fmaf(w, x * x, rxx);
                ryy = fmaf(w, y * y, ryy);
                rxy = fmaf(w, x * y, rxy);
            }
            mx = fmaf(g[i], rx, mx);
            my = fmaf(g[i], ry, my);
            mxx = fmaf(g[i], rxx, mxx);
            myy = fmaf(g[i], ryy, myy);
            mxy = fmaf(g[i], rxy, mxy);
        }
        const float sxx = mxx - mx * mx, syy = myy - my * my, sxy = mxy - mx * my;
        const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
        ss += (2.f * mx * my + c1) / (mx * mx + my * my + c1) * cs;
    }

    sq = wave_sum64(sq);
    ss = wave_sum64(ss);
    if ((t & 63) == 0) {
        red[0][t >> 6] = sq;
        red[1][t >> 6] = ss;
    }
    __syncthreads();
    if (t == 0) {
        const size_t at = (((size_t)n * C + c) * nb + b) * 2;
        ws[at + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        ws[at + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void metric_band_final_kernel(const float* __restrict__ ws,
                                                                float* __restrict__ psnr,
                                                                float* __restrict__ ssim, int N, int C,
                                                                int H, int W, int nb) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float sq = 0.f, ss = 0.f;
    for (int j = 0; j < C * nb; ++j) {
        sq += ws[((size_t)n * C * nb + j) * 2 + 0];
        ss += ws[((size_t)n * C * nb + j) * 2 + 1];
    }
    const float mse = sq / (float)(C * H * W);
    if (psnr) psnr[n] = 10.f * log10f(1.f / (mse + 1e-8f));
    if (ssim) ssim[n] = ss / (float)(C * (H - WIN + 1) * (W - WIN + 1));
}

constexpr size_t LDS_MAX = 160 * 1024 - 64;
constexpr size_t BAND_LDS = 64 * 1024;   // band size target: two workgroups per CU

bool fits_whole(int H, int W) { return (size_t)H * W * 2 * sizeof(float) <= LDS_MAX; }

// output rows per band (0: not even one band of 11 input rows fits)
int band_rows(int H, int W) {
    const size_t row_bytes = (size_t)W * 2 * sizeof(float);
    const int fit = (int)(LDS_MAX / row_bytes);
    if (fit < WIN) return 0;
    const int want = (int)(BAND_LDS / row_bytes);
    return min(H - WIN + 1, max(want, WIN) - (WIN - 1));
}

}  // namespace

extern "C" size_t tocvp_metrics_ws_bytes(int N, int C) {
    return (N > 0 && C > 0) ? (size_t)N * C * 2 * sizeof(float) : 0;
}

extern "C" size_t tocvp_metrics_ws_bytes_hw(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H < WIN || W < WIN) return 0;
    if (fits_whole(H, W)) return tocvp_metrics_ws_bytes(N, C);
    const int br = band_rows(H, W);
    if (br == 0) return 0;
    const int nb = (H - WIN + 1 + br - 1) / br;
    return (size_t)N * C * nb * 2 * sizeof(float);
}

extern "C" int tocvp_psnr_ssim_f32(const float* preds, const float* targets, float* psnr,
                                   float* ssim, int N, int C, int H, int W, int clamp01, void* ws,
                                   size_t ws_bytes, void* stream) {
    TOCVP_CHECK_ARG(preds && targets && (psnr || ssim) && ws);
    TOCVP_CHECK_ARG(N >= 0 && N <= 65535 * 256 && C > 0 && C <= 65535 && H >= WIN && W >= WIN);
    TOCVP_CHECK_ARG(N <= 65535);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!fits_whole(H, W)) {
        const int br = band_rows(H, W);
        TOCVP_CHECK_ARG(br > 0);
        if (N == 0) return TOCVP_OK;
        TOCVP_CHECK_ARG(ws_bytes >= tocvp_metrics_ws_bytes_hw(N, C, H, W));
        const int nb = (H - WIN + 1 + br - 1) / br;
        const size_t shm = (size_t)(min(br, H - WIN + 1) + WIN - 1) * W * 2 * sizeof(float);
        if (shm > 64 * 1024) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(metric_band_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
                return TOCVP_ELAUNCH;
        }
        hipLaunchKernelGGL(metric_band_kernel, dim3(nb, C, N), dim3(256), shm, s, preds, targets,
                           static_cast<float*>(ws), C, H, W, br, clamp01);
        if (hipGetLastError() != hipSuccess) return TOCVP_ELAUNCH;
        hipLaunchKernelGGL(metric_band_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s,
                           static_cast<const float*>(ws), psnr, ssim, N, C, H, W, nb);
        return tocvp_launch_status();
    }
    TOCVP_CHECK_ARG(ws_bytes >= tocvp_metrics_ws_bytes(N, C));
    if (N == 0) return TOCVP_OK;
    const size_t shm = (size_t)H * W * 2 * sizeof(float);
    if (shm > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(metric_partial_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
            return TOCVP_ELAUNCH;
    }
    hipLaunchKernelGGL(metric_partial_kernel, dim3(C, N), dim3(256), shm, s, preds, targets,
                       static_cast<float*>(ws), C, H, W, clamp01);
    if (hipGetLastError() != hipSuccess) return TOCVP_ELAUNCH;
    hipLaunchKernelGGL(metric_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s,
                       static_cast<const float*>(ws), psnr, ssim, N, C, H, W);
    return tocvp_launch_status();
}
