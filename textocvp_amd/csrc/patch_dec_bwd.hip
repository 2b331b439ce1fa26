// Backward of the frozen ExtendedDINOSAUR MLPPatchDecoder w.r.t. its slots (image-loss term of the predictor training
// step, reference models/EncodersDecoders/decoders.py:264-365 differentiated; the decoder's weights are frozen):
//
//  bilinear_resize_bwd_kernel : adjoint of F.interpolate(bilinear, align_corners=False) in GATHER form (every source
//                               pixel sums the output pixels whose taps read it: deterministic, no atomics), NCHW
//                               gradient in -> NHWC gradient out with zero padding channels (the layout the image head's
//                               final conv produced).
//  conv3x3_dgrad_kernel       : data gradient of a 3x3 conv (pad 1), or of "nearest x2 -> 3x3 conv", as an implicit GEMM
//                               over the gradient image, ReLU gate of the layer below applied in the store.
//                                 plain : dx[y][x] = sum_{dy,dx} g[y + dy - 1][x + dx - 1] . W'[dy][dx]   (9 taps)
//                                 up2   : dx[y][x] = sum_{r,s} g[2y + r - 1][2x + s - 1] . W'[r][s]       (16 taps)
//                               up2 is the adjoint of the four-phase conv3x3_up2: a stride-2 4x4 conv over the high-
//                               resolution gradient whose tap r sums the 3x3 rows {2-r, 3-r} & [0, 2] -- it writes the
//                               low-resolution input gradient directly (no full-resolution intermediate, no 2x2 sum-pool,
//                               16 tap products per input pixel like the forward).  Eval BatchNorm scale is folded into W'.
//                               ARITHMETIC: bf16x3 split operands (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16,
//                               ~2^-16 per product, fp32 accumulation).  Chosen over f16x3 planes with a measured operand
//                               scale because the incoming gradient is ~2 / numel (1e-8 at bench shapes) and spans many
//                               decades across a chunk: bf16 keeps the fp32 exponent range per element, so no device-
//                               side absmax pass, no scale and no flush of the small images' gradients.
//  slot_composite_bwd_kernel  : adjoint of the alpha-softmax + weighted feature sum, written into the zero-padded head
//                               layout (ld columns) that the head's data-gradient GEMM consumes as is.
//  ln_bcast_bwd_kernel        : LayerNorm(slot broadcast over the patches + position table) backward, summed over the
//                               patches per slot in a fixed order (the table is frozen: no gradient for it).
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 64, BK = 32, LDR = BK + 8;     // LDS row: 32 bf16 + 16 B pad (80 B)

struct DgradArgs {
    const float* g; const float* w; const float* gate; float* dx;
    int nimg, H, W, Cg, Cout;                                // H, W = size of dx (the conv's input)
};

__device__ __forceinline__ void split4(const f32x4 v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        hi[u] = (__bf16)v[u];
        lo[u] = (__bf16)(v[u] - (float)hi[u]);
    }
}

// Workgroup: 128 output pixels (flattened over images, rows, columns: any H, W) x 64 output channels, 4 waves of
// 32 pixels x 64 channels.  K loop: taps x 32-channel chunks of the gradient; A (gathered gradient pixels) and B
// (w (taps, Cout, Cg): K contiguous) are split into bf16 hi / lo while staged into LDS.
template <bool UP2>
__global__ __launch_bounds__(256) void conv3x3_dgrad_kernel(DgradArgs p) {
    constexpr int KS = UP2 ? 4 : 3, NT = KS * KS, ST = UP2 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) __bf16 a_hi[BM * LDR], a_lo[BM * LDR], b_hi[BN * LDR], b_lo[BN * LDR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const long P = (long)p.nimg * p.H * p.W;
    const long px0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int GH = p.H * ST, GW = p.W * ST;
    const int kc = (t & 7) * 4, row = t >> 3;                  // staging: 4 channels of row (t >> 3) + 32 it

    int ay[4], ax[4];
    size_t aimg[4];
    bool aok[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        long pp = px0 + row + 32 * it;
        aok[it] = pp < P;
        pp = aok[it] ? pp : 0;
        ax[it] = (int)(pp % p.W);
        ay[it] = (int)((pp / p.W) % p.H);
        aimg[it] = (size_t)(pp / ((long)p.W * p.H));
    }

    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    for (int tap = 0; tap < NT; ++tap) {
        const int ty = tap / KS, tx = tap % KS;
        const float* wt = p.w + (size_t)tap * p.Cout * p.Cg;
        for (int c0 = 0; c0 < p.Cg; c0 += BK) {
            f32x4 av[4], bv[2];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int sy = ay[it] * ST - 1 + ty, sx = ax[it] * ST - 1 + tx;
                const bool in = aok[it] && sy >= 0 && sy < GH && sx >= 0 && sx < GW;
                av[it] = in ? *reinterpret_cast<const f32x4*>(p.g + ((aimg[it] * GH + sy) * GW + sx) * p.Cg + c0 + kc)
                            : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int it = 0; it < 2; ++it)
                bv[it] = *reinterpret_cast<const f32x4*>(wt + (size_t)(n0 + row + 32 * it) * p.Cg + c0 + kc);
            __syncthreads();                                   // previous chunk consumed
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                bf16x4 hi, lo;
                split4(av[it], hi, lo);
                *reinterpret_cast<bf16x4*>(a_hi + (row + 32 * it) * LDR + kc) = hi;
                *reinterpret_cast<bf16x4*>(a_lo + (row + 32 * it) * LDR + kc) = lo;
            }
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                bf16x4 hi, lo;
                split4(bv[it], hi, lo);
                *reinterpret_cast<bf16x4*>(b_hi + (row + 32 * it) * LDR + kc) = hi;
                *reinterpret_cast<bf16x4*>(b_lo + (row + 32 * it) * LDR + kc) = lo;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                const int ao = (wave * 32 + l31) * LDR + ks * 16 + h * 8;
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + ao);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(a_lo + ao);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int bo = (n * 32 + l31) * LDR + ks * 16 + h * 8;
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(b_hi + bo);
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(b_lo + bo);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[n], 0, 0, 0);
                }
            }
        }
    }

#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int co = n0 + n * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long pix = px0 + wave * 32 + acc_row(r, h);
            if (pix < P) {
                const size_t o = (size_t)pix * p.Cout + co;
                float v = acc[n][r];
                if (p.gate) v = p.gate[o] > 0.f ? v : 0.f;
                p.dx[o] = v;
            }
        }
    }
}

// The forward's source coordinate of output row / column o (bilinear_resize_kernel, conv3x3.hip): taps i0, i1, weight l of i1
__device__ __forceinline__ void bilinear_taps(int o, float r, int S, int& i0, int& i1, float& l) {
    float f = ((float)o + 0.5f) * r - 0.5f;
    f = f < 0.f ? 0.f : f;
    i0 = (int)f;
    i1 = i0 + (i0 < S - 1 ? 1 : 0);
    l = f - (float)i0;
}

// weight of source index s in output index o, and whether o reads s at all (a zero weight still propagates NaN / inf,
// as the scatter form of the adjoint does)
__device__ __forceinline__ bool bilinear_weight(int o, float r, int S, int s, float& w) {
    int i0, i1;
    float l;
    bilinear_taps(o, r, S, i0, i1, l);
    w = (i0 == s ? 1.f - l : 0.f) + (i1 == s ? l : 0.f);
    return i0 == s || i1 == s;
}

// dy NCHW (n, C, OH, OW) -> dx NHWC (n, SH, SW, CSTR); channels [C, CSTR) written as zero
__global__ __launch_bounds__(256) void bilinear_resize_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                  int C, int CSTR, int SH, int SW, int OH, int OW,
                                                                  long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % CSTR);
    const int sx = (int)((i / CSTR) % SW), sy = (int)((i / ((long)CSTR * SW)) % SH);
    const long n = i / ((long)CSTR * SW * SH);
    float acc = 0.f;
    if (c < C) {
        const float ry = (float)SH / (float)OH, rx = (float)SW / (float)OW;
        // output rows whose first tap is sy - 1 or sy (the forward's taps are monotonic in o), with a margin of one;
        // from 0 for the first two rows (an upsampling forward clamps every row left of the first centre to row 0)
        const int ylo = sy <= 1 ? 0 : max(0, (int)floorf(((float)sy - 0.5f) / ry - 0.5f) - 1);
        const int yhi = min(OH - 1, (int)ceilf(((float)sy + 1.5f) / ry - 0.5f) + 1);
        const int xlo = sx <= 1 ? 0 : max(0, (int)floorf(((float)sx - 0.5f) / rx - 0.5f) - 1);
        const int xhi = min(OW - 1, (int)ceilf(((float)sx + 1.5f) / rx - 0.5f) + 1);
        const float* gp = dy + ((size_t)n * C + c) * OH * OW;
        for (int oy = ylo; oy <= yhi; ++oy) {
            float wy;
            if (!bilinear_weight(oy, ry, SH, sy, wy)) continue;
            float rowsum = 0.f;
            for (int ox = xlo; ox <= xhi; ++ox) {
                float wx;
                if (bilinear_weight(ox, rx, SW, sx, wx)) rowsum += wx * gp[(size_t)oy * OW + ox];
            }
            acc += wy * rowsum;
        }
    }
    dx[i] = acc;
}

// one workgroup per (patch n, frame b):  dfeat_k = alpha_k dR,  dlogit_k = alpha_k (<feat_k, dR> - sum_j alpha_j <feat_j, dR>)
__global__ __launch_bounds__(256) void slot_composite_bwd_kernel(const float* __restrict__ dR,
                                                                 const float* __restrict__ dec,
                                                                 const float* __restrict__ alpha,
                                                                 float* __restrict__ ddec, int K, int N, int F,
                                                                 int ld) {
    __shared__ float d_s[64], a_s[64];
    const int n = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* g = dR + ((size_t)b * N + n) * F;
    const size_t krow = (size_t)N * ld;
    const float* base = dec + ((size_t)b * K * N + n) * ld;
    float* obase = ddec + ((size_t)b * K * N + n) * ld;
    for (int k = wave; k < K; k += 4) {
        float s = 0.f;
        for (int f = lane; f < F; f += 64) s += base[k * krow + f] * g[f];
        s = wave_sum64(s);
        if (lane == 0) d_s[k] = s;
    }
    if (t < K) a_s[t] = alpha[((size_t)b * K + t) * N + n];
    __syncthreads();
    float mix = 0.f;
    for (int j = 0; j < K; ++j) mix += a_s[j] * d_s[j];
    for (int k = 0; k < K; ++k) {
        const float a = a_s[k];
        for (int f = t; f < ld; f += 256)
            obase[k * krow + f] = f < F ? a * g[f] : (f == F ? a * (d_s[k] - mix) : 0.f);
    }
}

// one workgroup per slot row s: x_n = slot[s] + pos[n], y_n = LN(x_n) gamma + beta;
// dslot[s] = sum_n dLN(dy[s, n]) (patches summed per wave in order, then the 4 waves in order)
template <int V>   // D / 64 values per lane
__global__ __launch_bounds__(256) void ln_bcast_bwd_kernel(const float* __restrict__ slots,
                                                           const float* __restrict__ pos,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ dy, float* __restrict__ dslot,
                                                           int N, int D, float eps) {
    __shared__ float red[4][V * 64];
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float sl[V], gm[V], acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        sl[v] = slots[(size_t)s * D + lane + 64 * v];
        gm[v] = gamma[lane + 64 * v];
        acc[v] = 0.f;
    }
    const float invD = 1.f / (float)D;
    for (int n = wave; n < N; n += 4) {
        float x[V], d[V], sum = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[v] = sl[v] + pos[(size_t)n * D + lane + 64 * v];
            d[v] = dy[((size_t)s * N + n) * D + lane + 64 * v] * gm[v];
            sum += x[v];
        }
        const float mean = wave_sum64(sum) * invD;
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[v] -= mean;
            q += x[v] * x[v];
        }
        const float rstd = 1.f / sqrtf(wave_sum64(q) * invD + eps);
        float sd = 0.f, sdx = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[v] *= rstd;                                      // x-hat
            sd += d[v];
            sdx += d[v] * x[v];
        }
        const float md = wave_sum64(sd) * invD, mdx = wave_sum64(sdx) * invD;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += rstd * (d[v] - md - x[v] * mdx);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) red[wave][lane + 64 * v] = acc[v];
    __syncthreads();
    for (int c = t; c < D; c += 256)
        dslot[(size_t)s * D + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

}  // namespace

extern "C" int tocvp_conv3x3_dgrad_bf16x3_f32(const float* g, const float* w, const float* gate, float* dx, int nimg,
                                              int H, int W, int Cg, int Cout, int up2, void* stream) {
    TOCVP_CHECK_ARG(g && w && dx);
    TOCVP_CHECK_ARG(nimg >= 0 && H > 0 && W > 0 && Cg > 0 && (Cg % BK) == 0 && Cout > 0 && (Cout % BN) == 0);
    const long P = (long)nimg * H * W;
    TOCVP_CHECK_ARG((P + BM - 1) / BM < 0x7fffffffL && Cout / BN <= 65535);
    if (!tocvp_aligned16(g) || !tocvp_aligned16(w)) return TOCVP_EALIGN;
    if (P == 0) return TOCVP_OK;
    DgradArgs a{g, w, gate, dx, nimg, H, W, Cg, Cout};
    const dim3 grid((unsigned)((P + BM - 1) / BM), Cout / BN);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (up2) hipLaunchKernelGGL(conv3x3_dgrad_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv3x3_dgrad_kernel<false>, grid, dim3(256), 0, s, a);
    return tocvp_launch_status();
}

extern "C" int tocvp_bilinear_resize_bwd_f32(const float* dy, float* dx, int n, int C, int cstride, int SH, int SW,
                                             int OH, int OW, void* stream) {
    TOCVP_CHECK_ARG(dy && dx && n >= 0 && C > 0 && cstride >= C && SH > 0 && SW > 0 && OH > 0 && OW > 0);
    const long total = (long)n * SH * SW * cstride;
    TOCVP_CHECK_ARG((total + 255) / 256 < 0x7fffffffL);
    if (total == 0) return TOCVP_OK;
    hipLaunchKernelGGL(bilinear_resize_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dy, dx, C, cstride, SH, SW, OH, OW, total);
    return tocvp_launch_status();
}

extern "C" int tocvp_slot_composite_bwd_f32(const float* dR, const float* decoded, const float* masks, float* ddec,
                                            int B, int K, int N, int F, int ld, void* stream) {
    TOCVP_CHECK_ARG(dR && decoded && masks && ddec);
    TOCVP_CHECK_ARG(B >= 0 && B <= 65535 && K > 0 && K <= 64 && N > 0 && F > 0 && ld >= F + 1);
    if (B == 0) return TOCVP_OK;
    hipLaunchKernelGGL(slot_composite_bwd_kernel, dim3(N, B), dim3(256), 0, static_cast<hipStream_t>(stream), dR,
                       decoded, masks, ddec, K, N, F, ld);
    return tocvp_launch_status();
}

extern "C" int tocvp_ln_bcast_bwd_f32(const float* slots, const float* pos, const float* gamma, const float* dy,
                                      float* dslot, int S, int N, int D, float eps, void* stream) {
    TOCVP_CHECK_ARG(slots && pos && gamma && dy && dslot);
    TOCVP_CHECK_ARG(S >= 0 && N > 0 && (D == 64 || D == 128 || D == 256 || D == 512));
    if (S == 0) return TOCVP_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)S);
    switch (D / 64) {
        case 1: hipLaunchKernelGGL(ln_bcast_bwd_kernel<1>, grid, dim3(256), 0, s, slots, pos, gamma, dy, dslot, N, D, eps); break;
        case 2: hipLaunchKernelGGL(ln_bcast_bwd_kernel<2>, grid, dim3(256), 0, s, slots, pos, gamma, dy, dslot, N, D, eps); break;
        case 4: hipLaunchKernelGGL(ln_bcast_bwd_kernel<4>, grid, dim3(256), 0, s, slots, pos, gamma, dy, dslot, N, D, eps); break;
        case 8: hipLaunchKernelGGL(ln_bcast_bwd_kernel<8>, grid, dim3(256), 0, s, slots, pos, gamma, dy, dslot, N, D, eps); break;
        default: return TOCVP_EINVAL;
    }
    return tocvp_launch_status();
}
