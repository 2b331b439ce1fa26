// LPIPS of the evaluation step (reference lib/metrics.py:259-298: piqa==1.2.2 `LPIPS(network="alex", pretrained=True,
// reduction=None)` on the clamped predictions and the targets, one value per image).  piqa is not vendored; its published
// definition (= the lpips package's v0.1 AlexNet metric) is restated:
//
//   x' = (clamp(x, 0, 1) - [0.485, 0.456, 0.406]) / [0.229, 0.224, 0.225] per channel
//        (algebraically the lpips ScalingLayer applied to 2x - 1)
//   torchvision alexnet().features, the five ReLU outputs tapped (zero padding applies to the SCALED input):
//     tap 1: conv 11x11 stride 4 pad 2, 3 -> 64,  ReLU      then max-pool 3 / 2
//     tap 2: conv 5x5  pad 2, 64 -> 192,  ReLU             then max-pool 3 / 2
//     tap 3: conv 3x3  pad 1, 192 -> 384, ReLU
//     tap 4: conv 3x3  pad 1, 384 -> 256, ReLU
//     tap 5: conv 3x3  pad 1, 256 -> 256, ReLU             (last pool and classifier unused)
//   per tap l: f_hat = f / (||f||_2 + 1e-10) over the channels of each pixel (LPIPS v0.1 epsilon),
//              d_l = mean_{h,w} sum_c w_{l,c} (fx_hat - fy_hat)^2 with the five 1x1 "lin" weights (no bias)
//   LPIPS = sum_l d_l.   H, W >= 31 (below 31 the second pool's output is empty).
//
// Unverified here: the epsilon inside piqa 1.2.2's normalisation.  It changes nothing at fp32 tolerance except at all-zero
// feature vectors, where this definition contributes w (0 - f_hat)^2 of the other image and piqa may give NaN if it has no
// epsilon.
//
//  lpips_conv_kernel   : one implicit-GEMM conv for all five layers on exact fp32 MFMA (v_mfma_f32_32x32x2_f32).  Rows are
//                        flattened (image, output pixel), columns Cout, K = kh * kw * Cin (k = (ky kw + kx) Cin + ci);
//                        64 x 64 tile per workgroup, 32-deep K slices staged in LDS, bias + ReLU epilogue, NHWC fp32 out.
//                        Flattening rows across images matters because the maps are tiny (15x15, 7x7, 3x3, 3x3, 3x3 at a
//                        64x64 input): conv3x3_mfma_kernel (conv3x3.hip) tiles 8 x 32 pixels of one image and needs
//                        H % 8 == 0, so it does not fit.  The first layer reads the NCHW frames in place from two base
//                        pointers (preds for images < nfirst, targets after) and fuses the clamp and the scaling: no
//                        2N-image copy and no scaled copy exist.
//  lpips_maxpool_kernel: max-pool 3 / 2 (no padding, floor) NHWC, a separate pass (simpler than folding nine loads into
//                        the conv loader; the pooled maps are small).
//  lpips_head_kernel   : one workgroup per (tap, image pair): normalisation, weighted squared difference, per-wave partial
//                        sums to the workspace; lpips_final_kernel adds them in a fixed order (no atomics: bitwise
//                        deterministic, and LPIPS(x, y) == LPIPS(y, x) bitwise since the features of an image do not depend
//                        on its row position and (a - b)^2 == (b - a)^2).
//
// Packed weights (tocvp_lpips_weights_floats() floats, packed by textocvp_amd.kernels.pack_lpips_weights): per layer l the
// matrix W_l[k][co] (k rows zero-padded to a multiple of 32) followed by bias_l[Cout], then the five lin vectors
// (64 + 192 + 384 + 256 + 256 floats).
#include "common.h"

namespace {

constexpr int NL = 5;
constexpr int KS_[NL] = {11, 5, 3, 3, 3};
constexpr int ST_[NL] = {4, 1, 1, 1, 1};
constexpr int PD_[NL] = {2, 2, 1, 1, 1};
constexpr int CI_[NL] = {3, 64, 192, 384, 256};
constexpr int CO_[NL] = {64, 192, 384, 256, 256};
constexpr int LIN_OFF_[NL] = {0, 64, 256, 640, 896};
constexpr int LIN_TOTAL = 1152;
constexpr int BM = 64, BN = 64, BK = 32;

constexpr int kdim(int l) { return KS_[l] * KS_[l] * CI_[l]; }
constexpr int kpad(int l) { return (kdim(l) + BK - 1) / BK * BK; }
constexpr size_t w_off(int l) { return l == 0 ? 0 : w_off(l - 1) + (size_t)(kpad(l - 1) + 1) * CO_[l - 1]; }
constexpr size_t b_off(int l) { return w_off(l) + (size_t)kpad(l) * CO_[l]; }
constexpr size_t lin_off() { return w_off(NL); }

__device__ __forceinline__ float scale_in(float v, int ci) {
    const float mean = ci == 0 ? 0.485f : (ci == 1 ? 0.456f : 0.406f);
    const float sd = ci == 0 ? 0.229f : (ci == 1 ? 0.224f : 0.225f);
    return (tocvp_clamp01(v) - mean) / sd;
}

// x: FIRST ? NCHW frames (3 channels; image i < nfirst from x, else x2 at i - nfirst) : NHWC (nimg, H, W, Cin).
// y: NHWC (nimg, OH, OW, Cout).  M = nimg * OH * OW.
template <int KS, int S, int P, bool FIRST>
__global__ __launch_bounds__(256) void lpips_conv_kernel(const float* __restrict__ x, const float* __restrict__ x2,
                                                         int nfirst, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, long M,
                                                         int H, int W, int OH, int OW, int Cin, int Cout, int K) {
    __shared__ __attribute__((aligned(16))) float As[BK][BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[BK][BN + 4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int ohw = OH * OW;

    // loader rows: FIRST -> one row (t & 63), k = kofs + 4 j; else two rows (t >> 3, + 32), one float4 of k each
    constexpr int NR = FIRST ? 1 : 2;
    const float* src[NR];
    int iy0[NR], ix0[NR];
    bool rv[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const int row = FIRST ? (t & 63) : (t >> 3) + 32 * u;
        const long m = m0 + row;
        rv[u] = m < M;
        const long mm = rv[u] ? m : 0;
        const long img = mm / ohw;
        const int r = (int)(mm - img * ohw), oy = r / OW, ox = r - (r / OW) * OW;
        iy0[u] = oy * S - P;
        ix0[u] = ox * S - P;
        if (FIRST)
            src[u] = img < nfirst ? x + (size_t)img * 3 * H * W : x2 + (size_t)(img - nfirst) * 3 * H * W;
        else
            src[u] = x + (size_t)img * H * W * Cin;
    }

    const int wm = wv & 1, wn = wv >> 1, li = lane & 31, lh = lane >> 5;
    f32x16 acc = {};
    const int kp = (K + BK - 1) / BK * BK;
    for (int k0 = 0; k0 < kp; k0 += BK) {
        if (FIRST) {
            const int row = t & 63, kofs = t >> 6;
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                const int kl = kofs + 4 * j, k = k0 + kl;
                float v = 0.f;
                if (rv[0] && k < K) {
                    const int tap = k / 3, ci = k - tap * 3, ky = tap / KS, kx = tap - ky * KS;
                    const int iy = iy0[0] + ky, ix = ix0[0] + kx;
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = scale_in(src[0][(size_t)ci * H * W + iy * W + ix], ci);
                }
                As[kl][row] = v;
            }
        } else {
            const int tap = k0 / Cin, ci0 = k0 - tap * Cin, ky = tap / KS, kx = tap - ky * KS, k4 = t & 7;
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int iy = iy0[u] + ky, ix = ix0[u] + kx;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (rv[u] && iy >= 0 && iy < H && ix >= 0 && ix < W)
                    v = *reinterpret_cast<const f32x4*>(src[u] + ((size_t)iy * W + ix) * Cin + ci0 + 4 * k4);
                const int row = (t >> 3) + 32 * u;
#pragma unroll
                for (int e = 0; e < 4; ++e) As[4 * k4 + e][row] = v[e];
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = t + 256 * u, kr = q >> 4, c4 = q & 15;
            *reinterpret_cast<f32x4*>(&Bs[kr][4 * c4]) =
                *reinterpret_cast<const f32x4*>(w + (size_t)(k0 + kr) * Cout + n0 + 4 * c4);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk)
            acc = mfma32(As[2 * kk + lh][wm * 32 + li], Bs[2 * kk + lh][wn * 32 + li], acc);
        __syncthreads();
    }

    const int col = n0 + wn * 32 + li;
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm * 32 + acc_row(r, lh);
        if (m < M) y[(size_t)m * Cout + col] = fmaxf(acc[r] + bv, 0.f);
    }
}

__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            long total, int H, int W, int C, int OH, int OW) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int C4 = C / 4;
    const int c4 = (int)(i % C4);
    long p = i / C4;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const long img = p / OH;
    const float* base = x + (((size_t)img * H + 2 * oy) * W + 2 * ox) * C + 4 * c4;
    f32x4 m = *reinterpret_cast<const f32x4*>(base);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((size_t)dy * W + dx) * C);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
        }
    *reinterpret_cast<f32x4*>(y + (size_t)i * 4) = m;
}

struct HeadTaps {
    size_t off[NL];   // float offset of tap l (image 0) in the workspace; image stride hw[l] * CO_[l]
    int hw[NL];
};

// grid (NL, npairs): pair p compares image p with image npairs + p of each tap
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ ws, const float* __restrict__ lin,
                                                         float* __restrict__ part, HeadTaps tp, int npairs) {
    const int l = blockIdx.x, p = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int C = CO_[l], HW = tp.hw[l], nc = C / 64;
    const float* fx = ws + tp.off[l] + (size_t)p * HW * C;
    const float* fy = ws + tp.off[l] + (size_t)(p + npairs) * HW * C;
    float wl[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) wl[j] = j < nc ? lin[LIN_OFF_[l] + 64 * j + lane] : 0.f;
    float acc = 0.f;
    for (int pix = wv; pix < HW; pix += 4) {
        float a[6], b[6], sx = 0.f, sy = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            a[j] = j < nc ? fx[(size_t)pix * C + 64 * j + lane] : 0.f;
            b[j] = j < nc ? fy[(size_t)pix * C + 64 * j + lane] : 0.f;
            sx = fmaf(a[j], a[j], sx);
            sy = fmaf(b[j], b[j], sy);
        }
        const float nx = sqrtf(wave_sum64(sx)) + 1e-10f, ny = sqrtf(wave_sum64(sy)) + 1e-10f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float d = a[j] / nx - b[j] / ny;
            acc = fmaf(wl[j], d * d, acc);
        }
    }
    acc = wave_sum64(acc);
    if (lane == 0) part[((size_t)p * NL + l) * 4 + wv] = acc;
}

__global__ __launch_bounds__(256) void lpips_final_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                          HeadTaps tp, int npairs) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npairs) return;
    float s = 0.f;
    for (int l = 0; l < NL; ++l) {
        const float* q = part + ((size_t)p * NL + l) * 4;
        s += ((q[0] + q[1]) + (q[2] + q[3])) / (float)tp.hw[l];
    }
    out[p] = s;
}

int conv_out(int n, int l) { return (n + 2 * PD_[l] - KS_[l]) / ST_[l] + 1; }
int pool_out(int n) { return n >= 3 ? (n - 3) / 2 + 1 : 0; }

// spatial sizes of the five taps and two pooled maps, and the workspace layout of tocvp_lpips_f32
struct Plan {
    int th[NL], tw[NL], ph[2], pw[2];
    size_t t_off[NL], p_off[2], part_off, floats;
};

Plan make_plan(int npairs, int H, int W) {
    Plan q{};
    const size_t nimg = 2 * (size_t)npairs;
    q.th[0] = conv_out(H, 0), q.tw[0] = conv_out(W, 0);
    q.ph[0] = pool_out(q.th[0]), q.pw[0] = pool_out(q.tw[0]);
    q.th[1] = conv_out(q.ph[0], 1), q.tw[1] = conv_out(q.pw[0], 1);
    q.ph[1] = pool_out(q.th[1]), q.pw[1] = pool_out(q.tw[1]);
    for (int l = 2; l < NL; ++l) q.th[l] = q.ph[1], q.tw[l] = q.pw[1];
    size_t o = 0;
    auto take = [&](size_t floats) { const size_t at = o; o += (floats + 63) / 64 * 64; return at; };
    q.t_off[0] = take(nimg * q.th[0] * q.tw[0] * CO_[0]);
    q.p_off[0] = take(nimg * q.ph[0] * q.pw[0] * CO_[0]);
    q.t_off[1] = take(nimg * q.th[1] * q.tw[1] * CO_[1]);
    q.p_off[1] = take(nimg * q.ph[1] * q.pw[1] * CO_[1]);
    for (int l = 2; l < NL; ++l) q.t_off[l] = take(nimg * q.th[l] * q.tw[l] * CO_[l]);
    q.part_off = take((size_t)npairs * NL * 4);
    q.floats = o;
    return q;
}

int launch_conv(int l, const float* x, const float* x2, int nfirst, const float* wpk, float* y, int nimg, int H, int W,
                hipStream_t s) {
    const int OH = conv_out(H, l), OW = conv_out(W, l);
    const long M = (long)nimg * OH * OW;
    if (M == 0) return TOCVP_OK;
    const dim3 grid((unsigned)((M + BM - 1) / BM), CO_[l] / BN);
    const float* w = wpk + w_off(l);
    const float* b = wpk + b_off(l);
    switch (l) {
        case 0:
            hipLaunchKernelGGL((lpips_conv_kernel<11, 4, 2, true>), grid, dim3(256), 0, s, x, x2, nfirst, w, b, y, M, H, W,
                               OH, OW, CI_[l], CO_[l], kdim(l));
            break;
        case 1:
            hipLaunchKernelGGL((lpips_conv_kernel<5, 1, 2, false>), grid, dim3(256), 0, s, x, x2, nfirst, w, b, y, M, H,
                               W, OH, OW, CI_[l], CO_[l], kdim(l));
            break;
        default:
            hipLaunchKernelGGL((lpips_conv_kernel<3, 1, 1, false>), grid, dim3(256), 0, s, x, x2, nfirst, w, b, y, M, H,
                               W, OH, OW, CI_[l], CO_[l], kdim(l));
            break;
    }
    return tocvp_launch_status();
}

int launch_pool(const float* x, float* y, int nimg, int H, int W, int C, hipStream_t s) {
    const int OH = pool_out(H), OW = pool_out(W);
    const long total = (long)nimg * OH * OW * (C / 4);
    if (total == 0) return TOCVP_OK;
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, total, H, W,
                       C, OH, OW);
    return tocvp_launch_status();
}

// bound on the rows of one conv launch (grid.x < 2^31) and on every index: 2^31 / 64 tiles of 64 rows
constexpr long MAX_ROWS = 1L << 36;

}  // namespace

extern "C" size_t tocvp_lpips_weights_floats(void) { return lin_off() + LIN_TOTAL; }

extern "C" size_t tocvp_lpips_ws_bytes(int npairs, int H, int W) {
    if (npairs <= 0 || H < 31 || W < 31) return 0;
    return make_plan(npairs, H, W).floats * sizeof(float);
}

extern "C" int tocvp_lpips_conv_f32(int layer, const float* x, const float* x2, int nfirst, const float* wpk, float* y,
                                    int nimg, int H, int W, void* stream) {
    TOCVP_CHECK_ARG(layer >= 0 && layer < NL && x && wpk && y && nimg >= 0 && H > 0 && W > 0);
    TOCVP_CHECK_ARG(conv_out(H, layer) > 0 && conv_out(W, layer) > 0);
    TOCVP_CHECK_ARG((long)nimg * conv_out(H, layer) * conv_out(W, layer) < MAX_ROWS);
    TOCVP_CHECK_ARG(tocvp_aligned16(wpk) && tocvp_aligned16(y));
    if (layer == 0)
        TOCVP_CHECK_ARG(nfirst >= 0 && nfirst <= nimg && (nfirst == nimg || x2));
    else
        TOCVP_CHECK_ARG(tocvp_aligned16(x));
    return launch_conv(layer, x, x2, nfirst, wpk, y, nimg, H, W, static_cast<hipStream_t>(stream));
}

extern "C" int tocvp_lpips_maxpool_f32(const float* x, float* y, int nimg, int H, int W, int C, void* stream) {
    TOCVP_CHECK_ARG(x && y && nimg >= 0 && H >= 3 && W >= 3 && C > 0 && C % 4 == 0);
    TOCVP_CHECK_ARG(tocvp_aligned16(x) && tocvp_aligned16(y));
    return launch_pool(x, y, nimg, H, W, C, static_cast<hipStream_t>(stream));
}

extern "C" int tocvp_lpips_f32(const float* preds, const float* targets, const float* wpk, float* out, int npairs,
                               int H, int W, void* ws, size_t ws_bytes, void* stream) {
    TOCVP_CHECK_ARG(preds && targets && wpk && out && ws && npairs >= 0 && npairs <= 65535 && H >= 31 && W >= 31);
    TOCVP_CHECK_ARG(tocvp_aligned16(wpk) && tocvp_aligned16(ws));
    if (npairs == 0) return TOCVP_OK;
    TOCVP_CHECK_ARG(ws_bytes >= tocvp_lpips_ws_bytes(npairs, H, W));
    const Plan q = make_plan(npairs, H, W);
    TOCVP_CHECK_ARG(2L * npairs * q.th[0] * q.tw[0] < MAX_ROWS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* f = static_cast<float*>(ws);
    const int nimg = 2 * npairs;
    int rc;
    if ((rc = launch_conv(0, preds, targets, npairs, wpk, f + q.t_off[0], nimg, H, W, s))) return rc;
    if ((rc = launch_pool(f + q.t_off[0], f + q.p_off[0], nimg, q.th[0], q.tw[0], CO_[0], s))) return rc;
    if ((rc = launch_conv(1, f + q.p_off[0], nullptr, 0, wpk, f + q.t_off[1], nimg, q.ph[0], q.pw[0], s))) return rc;
    if ((rc = launch_pool(f + q.t_off[1], f + q.p_off[1], nimg, q.th[1], q.tw[1], CO_[1], s))) return rc;
    if ((rc = launch_conv(2, f + q.p_off[1], nullptr, 0, wpk, f + q.t_off[2], nimg, q.ph[1], q.pw[1], s))) return rc;
    if ((rc = launch_conv(3, f + q.t_off[2], nullptr, 0, wpk, f + q.t_off[3], nimg, q.th[2], q.tw[2], s))) return rc;
    if ((rc = launch_conv(4, f + q.t_off[3], nullptr, 0, wpk, f + q.t_off[4], nimg, q.th[3], q.tw[3], s))) return rc;
    HeadTaps tp{};
    for (int l = 0; l < NL; ++l) tp.off[l] = q.t_off[l], tp.hw[l] = q.th[l] * q.tw[l];
    hipLaunchKernelGGL(lpips_head_kernel, dim3(NL, npairs), dim3(256), 0, s, f, wpk + lin_off(), f + q.part_off, tp,
                       npairs);
    if (hipGetLastError() != hipSuccess) return TOCVP_ELAUNCH;
    hipLaunchKernelGGL(lpips_final_kernel, dim3((npairs + 255) / 256), dim3(256), 0, s, f + q.part_off, out, tp, npairs);
    return tocvp_launch_status();
}
