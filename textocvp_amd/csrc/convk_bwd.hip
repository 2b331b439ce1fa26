// Backward of the frozen SAVi decoder variants (kernel 3 / 5 / 7, nearest x2 upsampling, eval batch-norm, widths 32 / 64 /
// 128; the generic path of ConvDecoder) w.r.t. the slots -- the image-loss term of the predictor training step:
//
//  convk_dgrad_kernel        : data gradient of a k x k conv (pad k / 2) over the gradient image, or of "nearest x2 -> k x k
//                              conv" (up2), as an implicit GEMM, ReLU gate of the layer below applied in the store.
//                                plain : dx[y][x] = sum_{ty,tx < k}  g[y + ty - r][x + tx - r] . W'[ty][tx]
//                                up2   : dx[y][x] = sum_{ty,tx < 2T} g[2y + ty - r][2x + tx - r] . W'[ty][tx]
//                              r = k / 2, T = r + 1.  up2 is the adjoint of the four phase convolutions of convk: a stride-2
//                              2T x 2T correlation over the high-resolution gradient that writes the low-resolution input
//                              gradient directly (tap t of an axis sums the k-taps d = a + 2r - t, a in {0, 1}; the
//                              host packs W', eval BatchNorm scale folded in).
//                              Tiling: a workgroup owns 8 x 16 output pixels of one image x 32 or 64 output channels.  Per
//                              channel chunk (32 gradient channels, 16 for up2) it stages the pixel tile plus its halo ONCE
//                              in LDS, split into bf16 hi / lo once, and runs every tap from there (the 3x3 kernel gathers
//                              A per tap from L2: 49-64 reads of each gradient pixel at k = 7).  The next chunk's halo is
//                              loaded into registers while the current one is multiplied.  Under up2 the halo columns are
//                              stored by parity (even columns, then odd): the lanes of a row read stride-2 columns, which
//                              then lie at consecutive LDS rows.  B (the weights) comes pre-split from L2 in 16-byte rows.
//                              ARITHMETIC: bf16x3 (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation),
//                              as conv3x3_dgrad: the incoming gradient is ~2 / numel and spans many decades, bf16 keeps the
//                              fp32 exponent range per element (no absmax pass, no operand scale).  No atomics, fixed
//                              summation order: bit-identical from run to run.
//  conv3x3_t4w_kernel        : the tail's transposed 3x3 conv, 4 -> C (C in {32, 64, 128}), ReLU gate of the last hidden
//                              activation, any H and W (tocvp_conv3x3_t4_f32 stops at C = 64 and W % 4 == 0).
//  dec_class_reduce_k_kernel : collapsed layer 0 (k x k border classes of conv.hip):
//                              dS[n, cls, c] = scale[c] * sum_{p in cls} g[n, p, c] * [(cpos[p, c] + S[n, cls, c]) * scale[c]
//                              + shift[c] > 0], per class in a fixed order (no atomics).
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int TY = 8, TX = 16;                               // output tile: 8 rows x 16 columns = 4 waves x 32 pixels

struct DgradKArgs {
    const float* g; const __bf16* whi; const __bf16* wlo; const float* gate; float* dx;
    int nimg, H, W, Cg, Cout, tiles_x, tiles_y;              // H, W = size of dx (the conv's input)
};

__device__ __forceinline__ void split4(const f32x4 v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        hi[u] = (__bf16)v[u];
        lo[u] = (__bf16)(v[u] - (float)hi[u]);
    }
}

template <int KS, bool UP2>
struct DgradGeom {
    static constexpr int R = KS / 2, ST = UP2 ? 2 : 1, NT = UP2 ? KS + 1 : KS;   // taps per axis
    static constexpr int CK = UP2 ? 16 : 32, LDR = CK + 8;                         // channels per chunk, LDS row (bf16)
    static constexpr int HY = ST * (TY - 1) + NT, HX = ST * (TX - 1) + NT;         // halo tile
    static constexpr int HXE = (HX + 1) / 2;                                        // even columns (up2 parity layout)
    static constexpr int NQ = CK / 4, ITEMS = HY * HX * NQ, NIT = (ITEMS + 255) / 256;
    static constexpr size_t LDS = (size_t)2 * HY * HX * LDR * sizeof(__bf16);
    __device__ static __forceinline__ int col(int hx) { return UP2 ? ((hx & 1) ? HXE : 0) + (hx >> 1) : hx; }
};

template <int KS, bool UP2, int NB>                         // NB = 32-channel output blocks per workgroup (1 or 2)
__global__ __launch_bounds__(256) void convk_dgrad_kernel(DgradKArgs p) {
    using G = DgradGeom<KS, UP2>;
    constexpr int NT = G::NT, CK = G::CK, LDR = G::LDR, HX = G::HX, NQ = G::NQ;
    __shared__ __attribute__((aligned(16))) __bf16 a_hi[G::HY * HX * LDR], a_lo[G::HY * HX * LDR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int tiles = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int ty0 = (tile / p.tiles_x) * TY, tx0 = (tile % p.tiles_x) * TX;
    const int n0 = blockIdx.y * (NB * 32);
    const int GH = p.H * G::ST, GW = p.W * G::ST;
    const int gy0 = ty0 * G::ST - G::R, gx0 = tx0 * G::ST - G::R;      // gradient pixel of halo (0, 0)
    const float* gimg = p.g + (size_t)img * GH * GW * p.Cg;

    // staging items of this thread: (halo pixel, 4-channel quad); the same items for every chunk
    int soff[G::NIT], goff[G::NIT];                         // LDS element offset (-1: none), gradient offset (-1: zero)
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
        const int i = t + 256 * it;
        const int q = i % NQ, hp = i / NQ, hy = hp / HX, hx = hp % HX;
        const int gy = gy0 + hy, gx = gx0 + hx;
        soff[it] = i < G::ITEMS ? (hy * HX + G::col(hx)) * LDR + 4 * q : -1;
        goff[it] = (i < G::ITEMS && gy >= 0 && gy < GH && gx >= 0 && gx < GW) ? (gy * GW + gx) * p.Cg + 4 * q : -1;
    }
    f32x4 pre[G::NIT];
    auto load = [&](int c0) {
#pragma unroll
        for (int it = 0; it < G::NIT; ++it)
            pre[it] = goff[it] >= 0 ? *reinterpret_cast<const f32x4*>(gimg + goff[it] + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // this lane's A row: output pixel (oy, ox) of the tile
    const int oy = wave * 2 + (l31 >> 4), ox = l31 & 15;
    f32x16 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    load(0);
    for (int c0 = 0; c0 < p.Cg; c0 += CK) {
        __syncthreads();                                     // previous chunk consumed
#pragma unroll
        for (int it = 0; it < G::NIT; ++it) {
            if (soff[it] < 0) continue;
            bf16x4 hi, lo;
            split4(pre[it], hi, lo);
            *reinterpret_cast<bf16x4*>(a_hi + soff[it]) = hi;
            *reinterpret_cast<bf16x4*>(a_lo + soff[it]) = lo;
        }
        __syncthreads();
        if (c0 + CK < p.Cg) load(c0 + CK);                  // in flight during this chunk's products
        for (int ty = 0; ty < NT; ++ty) {
            const int arow = (G::ST * oy + ty) * HX;
#pragma unroll
            for (int tx = 0; tx < NT; ++tx) {
                const int tap = ty * NT + tx;
                const int ab = (arow + G::col(G::ST * ox + tx)) * LDR + h * 8;
#pragma unroll
                for (int ks = 0; ks < CK / 16; ++ks) {
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + ab + ks * 16);
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(a_lo + ab + ks * 16);
#pragma unroll
                    for (int n = 0; n < NB; ++n) {
                        const size_t wo = ((size_t)tap * p.Cout + n0 + n * 32 + l31) * p.Cg + c0 + ks * 16 + h * 8;
                        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(p.whi + wo);
                        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(p.wlo + wo);
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[n], 0, 0, 0);
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[n], 0, 0, 0);
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[n], 0, 0, 0);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const int co = n0 + n * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pi = acc_row(r, h);
            const int y = ty0 + wave * 2 + (pi >> 4), x = tx0 + (pi & 15);
            if (y < p.H && x < p.W) {
                const size_t o = (((size_t)img * p.H + y) * p.W + x) * p.Cout + co;
                float v = acc[n][r];
                if (p.gate) v = p.gate[o] > 0.f ? v : 0.f;
                p.dx[o] = v;
            }
        }
    }
}

// dx[n,y,x,ci] = relu'(act[n,y,x,ci]) * sum_{ty, tx, co < 4} w[co,ci,ty,tx] * dy[n, y+1-ty, x+1-tx, co], summed in the
// order of conv3x3_t4_kernel (train.hip).  Item = (4 consecutive pixels of a row, 4 channels), the last quad of a row
// partial when W % 4 != 0; w (4, C, 3, 3) staged once per workgroup in LDS as [tap][co][C].
__global__ __launch_bounds__(256) void conv3x3_t4w_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          const float* __restrict__ act, float* __restrict__ dx,
                                                          long nitem, int H, int W, int C) {
    __shared__ __attribute__((aligned(16))) float ws[9 * 4 * 128];
    for (int i = threadIdx.x; i < 9 * 4 * C; i += 256) {
        const int c = i % C, co = (i / C) & 3, tap = i / (4 * C);
        ws[i] = w[((size_t)co * C + c) * 9 + tap];
    }
    __syncthreads();
    const int cq = C / 4, wq = (W + 3) / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nitem; i += (long)gridDim.x * 256) {
        const long quad = i / cq;
        const int c4 = (int)(i % cq) * 4;
        const int x0 = (int)(quad % wq) * 4, y = (int)((quad / wq) % H);
        const long n = quad / ((long)wq * H);
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
            const int yy = y + 1 - ty;
            if (yy < 0 || yy >= H) continue;
            const float* row = dy + ((size_t)n * H + yy) * W * 4;
            f32x4 g[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int xx = x0 - 1 + j;
                g[j] = (xx >= 0 && xx < W) ? *reinterpret_cast<const f32x4*>(row + (size_t)xx * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                for (int co = 0; co < 4; ++co) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + ((ty * 3 + tx) * 4 + co) * C + c4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] += wv * g[q + 2 - tx][co];
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (x0 + q >= W) break;
            const size_t o = (((size_t)n * H + y) * W + x0 + q) * C + c4;
            const f32x4 a = *reinterpret_cast<const f32x4*>(act + o);
            f32x4 v = acc[q];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = a[u] > 0.f ? v[u] : 0.f;
            *reinterpret_cast<f32x4*>(dx + o) = v;
        }
    }
}

// class cls of one axis (border_class_k / classk_range of conv.hip): the pixels [lo, hi] whose class it is
__device__ __forceinline__ void class_pixels(int cls, int n, int ks, int& lo, int& hi) {
    const int r = ks / 2;
    if (cls < r) lo = hi = cls;
    else if (cls > r) lo = hi = n - ks + cls;
    else { lo = r; hi = n - 1 - r; }
}

// one workgroup per slot image; thread = (pixel lane pl, channel quad); per class: each lane sums its pixels in row-major
// order, then the lanes are summed in order through LDS
__global__ __launch_bounds__(256) void dec_class_reduce_k_kernel(const float* __restrict__ g, const float* __restrict__ cpos,
                                                                 const float* __restrict__ S, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float* __restrict__ dS,
                                                                 int H, int W, int C, int ks) {
    __shared__ __attribute__((aligned(16))) float part[256 * 4];
    const int n = blockIdx.x, t = threadIdx.x;
    const int cq = C / 4, PL = 256 / cq;
    const int c4 = (t % cq) * 4, pl = t / cq;
    const float* gn = g + (size_t)n * H * W * C;
    const float* Sn = S + (size_t)n * ks * ks * C;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f};
    if (scale) sc = *reinterpret_cast<const f32x4*>(scale + c4);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c4);
    for (int cls = 0; cls < ks * ks; ++cls) {
        int ylo, yhi, xlo, xhi;
        class_pixels(cls / ks, H, ks, ylo, yhi);
        class_pixels(cls % ks, W, ks, xlo, xhi);
        const int ncol = xhi - xlo + 1, npx = (yhi - ylo + 1) * ncol;
        const f32x4 sv = *reinterpret_cast<const f32x4*>(Sn + (size_t)cls * C + c4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = pl; i < npx; i += PL) {
            const size_t pix = (size_t)(ylo + i / ncol) * W + xlo + i % ncol;
            const f32x4 gv = *reinterpret_cast<const f32x4*>(gn + pix * C + c4);
            const f32x4 cp = *reinterpret_cast<const f32x4*>(cpos + pix * C + c4);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += fmaf(cp[u] + sv[u], sc[u], sh[u]) > 0.f ? gv[u] : 0.f;
        }
        *reinterpret_cast<f32x4*>(part + pl * C + c4) = acc;
        __syncthreads();
        if (t < C) {
            float s = 0.f;
            for (int j = 0; j < PL; ++j) s += part[j * C + t];
            dS[((size_t)n * ks * ks + cls) * C + t] = scale ? scale[t] * s : s;
        }
        __syncthreads();
    }
}

template <int KS, bool UP2, int NB>
int launch_dgrad(const DgradKArgs& a, unsigned nblk, hipStream_t s) {
    constexpr size_t lds = DgradGeom<KS, UP2>::LDS;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    hipLaunchKernelGGL((convk_dgrad_kernel<KS, UP2, NB>), dim3(nblk, a.Cout / (NB * 32)), dim3(256), 0, s, a);
    return tocvp_launch_status();
}

template <int KS, bool UP2>
int dispatch_nb(const DgradKArgs& a, unsigned nblk, hipStream_t s) {
    return a.Cout == 32 ? launch_dgrad<KS, UP2, 1>(a, nblk, s) : launch_dgrad<KS, UP2, 2>(a, nblk, s);
}

inline bool savi_width(int c) { return c == 32 || c == 64 || c == 128; }

}  // namespace

extern "C" int tocvp_convk_dgrad_bf16x3_f32(const float* g, const void* wsplit, const float* gate, float* dx, int nimg,
                                            int H, int W, int Cg, int Cout, int ksize, int up2, void* stream) {
    TOCVP_CHECK_ARG(g && wsplit && dx && (ksize == 3 || ksize == 5 || ksize == 7) && (up2 == 0 || up2 == 1));
    TOCVP_CHECK_ARG(nimg >= 0 && H > 0 && W > 0 && savi_width(Cg) && savi_width(Cout));
    const long tiles = (long)((H + TY - 1) / TY) * ((W + TX - 1) / TX);
    TOCVP_CHECK_ARG(tiles * nimg < 0x7fffffffL && (long)H * W * Cg * (up2 ? 4 : 1) < 0x7fffffffL);
    if (!tocvp_aligned16(g) || !tocvp_aligned16(wsplit)) return TOCVP_EALIGN;
    if (nimg == 0) return TOCVP_OK;
    const int nt = up2 ? ksize + 1 : ksize;
    const __bf16* whi = static_cast<const __bf16*>(wsplit);
    DgradKArgs a{g, whi, whi + (size_t)nt * nt * Cout * Cg, gate, dx, nimg, H, W, Cg, Cout, (W + TX - 1) / TX,
                 (H + TY - 1) / TY};
    const unsigned nblk = (unsigned)(tiles * nimg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (ksize * 2 + up2) {
        case 6: return dispatch_nb<3, false>(a, nblk, s);
        case 7: return dispatch_nb<3, true>(a, nblk, s);
        case 10: return dispatch_nb<5, false>(a, nblk, s);
        case 11: return dispatch_nb<5, true>(a, nblk, s);
        case 14: return dispatch_nb<7, false>(a, nblk, s);
        default: return dispatch_nb<7, true>(a, nblk, s);
    }
}

extern "C" int tocvp_conv3x3_t4w_f32(const float* dy, const float* w, const float* act, float* dx, int nimg, int H, int W,
                                     int C, void* stream) {
    TOCVP_CHECK_ARG(dy && w && act && dx && nimg >= 0 && H > 0 && W > 0 && savi_width(C));
    if (!tocvp_aligned16(dy) || !tocvp_aligned16(act) || !tocvp_aligned16(dx)) return TOCVP_EALIGN;
    const long nitem = (long)nimg * H * ((W + 3) / 4) * (C / 4);
    if (nitem == 0) return TOCVP_OK;
    const long want = (nitem + 255) / 256;
    hipLaunchKernelGGL(conv3x3_t4w_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dy, w, act, dx, nitem, H, W, C);
    return tocvp_launch_status();
}

extern "C" int tocvp_dec_class_reduce_k_f32(const float* g, const float* cpos, const float* S, const float* scale,
                                            const float* shift, float* dS, int nimg, int H, int W, int C, int ksize,
                                            void* stream) {
    TOCVP_CHECK_ARG(g && cpos && S && shift && dS && (ksize == 3 || ksize == 5 || ksize == 7));
    TOCVP_CHECK_ARG(nimg >= 0 && nimg <= 0x7fffffff && H >= ksize && W >= ksize && savi_width(C));
    if (!tocvp_aligned16(g) || !tocvp_aligned16(cpos) || !tocvp_aligned16(S) || !tocvp_aligned16(shift) ||
        (scale && !tocvp_aligned16(scale)))
        return TOCVP_EALIGN;
    if (nimg == 0) return TOCVP_OK;
    hipLaunchKernelGGL(dec_class_reduce_k_kernel, dim3((unsigned)nimg), dim3(256), 0, static_cast<hipStream_t>(stream), g,
                       cpos, S, scale, shift, dS, H, W, C, ksize);
    return tocvp_launch_status();
}
