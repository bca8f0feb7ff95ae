// Input gradients of the NLL at coupling widths 33 .. 512 on the f32 matrix cores of gfx950 (nf_nll_grad with NF_CFG_GRAD_GEMM).
//
// The contract of nf_grad_kernel (nf_grad.hip) and the reversible sweep of nf_grad_wide.hip in the geometry of nf_gemm_kernel
// (nf_gemm.hip, variant A): one workgroup of 512 threads per patch of up to 32x32 pixels, grid-stride over patches; thread t owns
// the pixels t and t + 512 (their z, g = d nll / d z and gy live in its registers); the coupling CNN at the padded width WP runs
// BAND by band (NB = 32768 / WP pixels, the band's activations in LDS in B-operand order), weights streamed from L2 in fetch order
// (nf_gemm_layout.h, NFGG_*).
//   forward sweep   per coupling and band: l_1 (K = 18) -> ReLU -> LDS; l_2 (the WP x WP product: 2 x 2 accumulator tiles per
//                   wavefront) -> ReLU -> P = W3^T relu(h2) per wavefront, the WM partial records summed by the 9-tap gather.  The
//                   sign of every D register of h1 and h2 goes to the gate record: 16 bits per lane and tile, in device scratch of
//                   THIS WORKGROUP (not per patch: a workgroup holds one patch at a time).  z, nll_b as nf_grad_kernel forms them.
//   backward sweep  g = z, then the ops in reverse; every op rebuilds its input from its output, then transforms g.  A coupling
//                   runs the forward chain again on the rebuilt z0 tile with the RECORDED gates (shift, ls), publishes d(shift, raw)
//                   into a zero-bordered tile and runs the three transposed products band by band:
//                   d h2 = W3 G36 (K = 36, B operands read at the nine taps of that tile) -> gate 2 -> LDS;
//                   d h1 = W2^T d h2 (the second WP x WP product, same loop) -> gate 1 -> D18 = W1 d h1 per wavefront; the WM partial
//                   records are summed by the scatter-gather of the nine taps into g0.
// 'SAME' padding: the zero borders of the two tiles and the bounds checks of the two gathers.  The border table E is constant and has
// no gradient.  Everything in front of the first coupling is computed forward from the loaded x.
// Beyond 32x32 (NF_CFG_GRAD_TILED_GEMM) the TILED instantiations run the same sweeps on one tile of an image and one segment of the
// program per launch patch, as nf_grad_wide_kernel<.., TILED> does at width 32.
// Conditioning, loads and the pointwise layers in the NLL direction are nf_grad_common.h's GradFrame, as in every gradient kernel.
// Weights are not staged in LDS at any width: the band takes 128 KiB of the CU's 160, every weight is consumed by exactly one
// wavefront of the workgroup, and at widths 64 / 128 a coupling's block (66 / 195 KiB) is L2-resident like the 2.3 MiB at 512.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "nf_device.h"
#include "nf_gemm_layout.h"
#include "nf_dev_util.h"
#include "nf_internal.h"
#include "nf_gemm_common.h"   // GT, GW, v16f, ldg4, gemm_acc_bias
#include "nf_grad_common.h"   // GradFrame

namespace {

__device__ __forceinline__ float gg_gate(uint32_t word, int bit, float x) { return ((word >> bit) & 1u) ? x : 0.0f; }
__device__ __forceinline__ uint32_t gg_signs(const v16f &d)
{
    uint32_t w = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) w |= (__float_as_int(d[v]) > 0 ? 1u : 0u) << v;
    return w;
}

// The WP x WP product of a band: this wavefront's 2 x 2 accumulator tiles over the whole K.  A operands (ap0 / ap1: the two channel
// tiles' images, chunk kc of 4 K steps at + 256 kc floats) from L2, B operands (bp0 / bp1: the two pixel tiles, chunk kc at
// + 8 NB kc floats) from LDS; the software pipeline of nf_gemm_kernel: the loads of chunk kc + 1 are issued before the 16 MFMAs of kc.
template <int KC, int NB>
__device__ __forceinline__ void gg_l2(v16f (&acc)[2][2], const float *ap0, const float *ap1, const float *bp0, const float *bp1)
{
    float4 xa0 = ldg4(ap0), xa1 = ldg4(ap1);
    float4 xb0 = *reinterpret_cast<const float4 *>(bp0), xb1 = *reinterpret_cast<const float4 *>(bp1);
    float4 ya0, ya1, yb0, yb1;
#define NF_GG_CHUNK(A0, A1, B0, B1)                                                                                \
    {                                                                                                              \
        const float as0[4] = {A0.x, A0.y, A0.z, A0.w}, as1[4] = {A1.x, A1.y, A1.z, A1.w};                          \
        const float bs0[4] = {B0.x, B0.y, B0.z, B0.w}, bs1[4] = {B1.x, B1.y, B1.z, B1.w};                          \
        _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                              \
        {                                                                                                          \
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(as0[s], bs0[s], acc[0][0], 0, 0, 0);                  \
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(as0[s], bs1[s], acc[0][1], 0, 0, 0);                  \
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(as1[s], bs0[s], acc[1][0], 0, 0, 0);                  \
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(as1[s], bs1[s], acc[1][1], 0, 0, 0);                  \
        }                                                                                                          \
    }
#pragma unroll 1
    for (int kc = 0; kc < KC; kc += 2) {
        const int k1 = kc + 1, k2 = kc + 2 < KC ? kc + 2 : KC - 1;
        ya0 = ldg4(ap0 + (size_t)k1 * 256);
        ya1 = ldg4(ap1 + (size_t)k1 * 256);
        yb0 = *reinterpret_cast<const float4 *>(bp0 + (size_t)k1 * 2 * NB * 4);
        yb1 = *reinterpret_cast<const float4 *>(bp1 + (size_t)k1 * 2 * NB * 4);
        __builtin_amdgcn_sched_barrier(0);
        NF_GG_CHUNK(xa0, xa1, xb0, xb1)
        __builtin_amdgcn_sched_barrier(0);
        xa0 = ldg4(ap0 + (size_t)k2 * 256);
        xa1 = ldg4(ap1 + (size_t)k2 * 256);
        xb0 = *reinterpret_cast<const float4 *>(bp0 + (size_t)k2 * 2 * NB * 4);
        xb1 = *reinterpret_cast<const float4 *>(bp1 + (size_t)k2 * 2 * NB * 4);
        __builtin_amdgcn_sched_barrier(0);
        NF_GG_CHUNK(ya0, ya1, yb0, yb1)
        __builtin_amdgcn_sched_barrier(0);
    }
#undef NF_GG_CHUNK
}

//   WP       padded coupling width: 64, 128, 256, 512
//   scratch  the gate records of the launch, `scratch_halves` uint16 per workgroup (nfgg_gate_halves)
//   TILED    NF_CFG_GRAD_TILED_GEMM (nf_device.h, "gradient tiles"), the contract of nf_grad_wide_kernel<.., TILED>: a "patch" of the
//            launch is one H x W tile of an img_H x img_W image and `prog` one segment.  Addresses and the index into the border table
//            E follow the IMAGE (recomputed from the tile's origin where they are used); the zero borders of the two LDS tiles and
//            the bounds checks of the gathers stay the TILE's — a tile is evaluated on its own, the wrong terms stay inside the
//            halo — and only the core window is stored.  nll_b is not formed here.  The gate record is one segment's.
template <int WP, bool TILED = false>
__global__ __launch_bounds__(GT) void nf_grad_gemm_kernel(const NfProgram prog, const NfGradLaunch a, uint16_t *const scratch, const size_t scratch_halves)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int OWN = 2;                 // pixels per thread: patches of up to 1024 pixels
    constexpr int MT = WP / 32;            // channel tiles
    constexpr int NB = NF7_BAND_FLOATS / WP;   // pixels per band
    constexpr int NT = NB / 32;            // pixel tiles per band
    constexpr int WM = MT / 2;             // wavefronts along the channel axis of the WP x WP products (2 tiles each)
    constexpr int WN = GW / WM;            // wavefronts along the pixel axis (2 tiles each)
    constexpr int KC = WP / 8;             // chunks of 4 K steps (8 input channels)
    static_assert(MT * NT == 32 && WM * WN == GW && NT == 2 * WN && KC % 2 == 0, "tile split");
    static_assert(WM * NB * NF7_P_STRIDE <= NF7_BAND_FLOATS && WM * NB * NFGG_D_STRIDE <= NF7_BAND_FLOATS, "the partial records reuse the band");
    const int H = a.H, W = a.W, HW = H * W;
    const int Wp = W + 2;
    const int PL = nfgg_plane(H, W);
    float *const band = smem;                        // [KC][2][NB][4]; later the partial P / D18 records [WM][NB][stride]
    float *const z0s = smem + NF7_BAND_FLOATS;       // [2][PL] channel planes of the pass-through half
    float *const dts = z0s + 2 * PL;                 // [4][PL] planes of d(shift, raw)
    float *const red = dts + 4 * PL;                 // [2][GW]

    const int t = threadIdx.x;
    const int wv = t >> 6, lane = t & 63, n = lane & 31, g = lane >> 5;
    const int wm = wv / WN, wn = wv % WN;
    const int n_bands = (HW + NB - 1) / NB;
    uint16_t *const gates = scratch + (size_t)blockIdx.x * scratch_halves;
    // 16 gate bits of this lane for (coupling, band, layer 0 = h1 / 1 = h2, tile m * NT + nt)
    auto gate_at = [&](int cidx, int bnd, int layer, int tile) { return gates + ((((size_t)cidx * n_bands + bnd) * 2 + layer) * 32 + tile) * 64 + lane; };

    // zero both tiles once: the borders are never written again
    for (int i = t; i < 6 * PL; i += GT) z0s[i] = 0.0f;
    __syncthreads();

    int pr[OWN], pc[OWN], lidx[OWN], bmask[OWN];
    bool act[OWN];
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const int p = t + GT * m;
        act[m] = p < HW;
        pr[m] = act[m] ? p / W : 0;
        pc[m] = act[m] ? p - pr[m] * W : 0;
        lidx[m] = (pr[m] + 1) * Wp + pc[m] + 1;
        bmask[m] = act[m] ? ((pr[m] == 0 ? 1 : 0) | (pr[m] == H - 1 ? 2 : 0) | (pc[m] == 0 ? 4 : 0) | (pc[m] == W - 1 ? 8 : 0)) : 0;
    }

    const int n_ops = prog.n_ops;
    const int first_cpl = a.first_cpl;
    // TILED: where the tile of the current launch patch sits in its image (wave-uniform), and what follows from it per owned pixel
    [[maybe_unused]] int oy = 0, ox = 0, cy0 = 0, cy1 = 0, cx0 = 0, cx1 = 0;
    auto gidx_of = [&](int m) {   // the pixel's index in the patch's / image's tensors (act[m] pixels only)
        if constexpr (TILED) return (oy + pr[m]) * a.img_W + ox + pc[m];
        else return t + GT * m;
    };
    auto bmask_of = [&](int m) {
        if constexpr (TILED) {
            const int R = oy + pr[m], C = ox + pc[m];
            return act[m] ? ((R == 0 ? 1 : 0) | (R == a.img_H - 1 ? 2 : 0) | (C == 0 ? 4 : 0) | (C == a.img_W - 1 ? 8 : 0)) : 0;
        } else {
            return bmask[m];
        }
    };
    [[maybe_unused]] auto own_of = [&](int m) {   // TILED: the pixel is in the tile's core window
        const int R = oy + pr[m], C = ox + pc[m];
        return act[m] && R >= cy0 && R < cy1 && C >= cx0 && C < cx1;
    };

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        int64_t img = b;
        if constexpr (TILED) {   // tile b % tiles of image b / tiles (nf_device.h, "overlapping tiles")
            const int nt = a.tile_ny * a.tile_nx;
            img = b / nt;
            const int ti = (int)(b - img * nt);
            const int ty = ti / a.tile_nx, tx = ti - ty * a.tile_nx;
            oy = nf_tile_origin(ty, a.img_H, H, a.tile_halo);
            ox = nf_tile_origin(tx, a.img_W, W, a.tile_halo);
            cy0 = nf_tile_core0(ty, a.img_H, H, a.tile_halo);
            cy1 = nf_tile_core1(ty, a.tile_ny, a.img_H, H, a.tile_halo);
            cx0 = nf_tile_core0(tx, a.img_W, W, a.tile_halo);
            cx1 = nf_tile_core1(tx, a.tile_nx, a.img_W, W, a.tile_halo);
        }
        const size_t patch_off = TILED ? (size_t)img * (size_t)a.img_H * (size_t)a.img_W : (size_t)b * (size_t)HW;
        const float4 *const x4 = reinterpret_cast<const float4 *>(TILED ? a.z_in : a.x) + patch_off;
        const float4 *const y4 = reinterpret_cast<const float4 *>(a.y) + patch_off;   // (not dereferenced when a.y is null)
        const nf_crow_p crow = (nf_crow_p)(a.cond_rows) + img;
        const GradPix<OWN, decltype(gidx_of)> pix = {act, gidx_of};
        const GradFrame<OWN, NfGradLaunch, GradPix<OWN, decltype(gidx_of)>> F = {prog, a, pix, crow, patch_off, x4, y4};

        // The coupling CNN on z0 = z[.][0:2]: o = (shift, raw log-scale) of the owned pixels.  RECORD: the forward sweep — ReLU by
        // sign, gate bits written; otherwise the backward sweep's recomputation on the rebuilt z0 — ReLU by the recorded bits.
        // Ends behind a barrier: every LDS read of the z0 tile and of the band is done.
        auto coupling_cnn = [&](int off, int cidx, auto record, const float (&z)[OWN][4], float (&o)[OWN][4]) {
            constexpr bool RECORD = decltype(record)::value;
            const float *const img = a.params + off + NFGG_CPL_FWD;
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                if (act[m]) {
                    z0s[lidx[m]] = z[m][0];
                    z0s[PL + lidx[m]] = z[m][1];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) o[m][j] = 0.0f;
            }
            __syncthreads();

            for (int bnd = 0; bnd < n_bands; ++bnd) {
                const int p0 = bnd * NB;
                // ---- l_1: 32 tiles of h1 = relu(W1 z0 + b1), 4 per wavefront, into LDS in B-operand order ----
#pragma unroll 1
                for (int i = 0; i < 4; ++i) {
                    const int tt = wv * 4 + i, m = tt / NT, nt = tt % NT;
                    if (p0 + 32 * nt >= HW) continue;   // wave-uniform: a pixel tile past the patch is never gathered
                    int p = p0 + 32 * nt + n;
                    p = p < HW ? p : HW - 1;
                    const int r = p / W, c = p - r * W;
                    const float *zb = z0s + g * PL + r * Wp + c;   // tap (di,dj) at + di*Wp + dj
                    v16f d = gemm_acc_bias(img + nf7_img_B1(WP) + m * 32 + g * 16);
#pragma unroll
                    for (int grp = 0; grp < 3; ++grp) {
                        const float4 aw = ldg4(img + nf7_img_A1(WP) + ((m * 3 + grp) * 64 + lane) * 4);
                        const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int tap = grp * 4 + s;
                            if (tap < 9) d = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], zb[(tap / 3) * Wp + tap % 3], d, 0, 0, 0);
                        }
                    }
                    uint16_t *const gp = gate_at(cidx, bnd, 0, tt);
                    uint32_t gw;
                    if constexpr (RECORD) {
                        gw = gg_signs(d);
                        *gp = (uint16_t)gw;
                    } else {
                        gw = *gp;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4 *>(band + ((((m * 4 + q) * 2 + g) * NB) + 32 * nt + n) * 4) =
                            make_float4(gg_gate(gw, 4 * q + 0, d[4 * q + 0]), gg_gate(gw, 4 * q + 1, d[4 * q + 1]), gg_gate(gw, 4 * q + 2, d[4 * q + 2]),
                                        gg_gate(gw, 4 * q + 3, d[4 * q + 3]));
                }
                __syncthreads();

                // ---- l_2 and P = W3^T relu(h2): this wavefront's 64 channels x 64 pixels ----
                const bool live = p0 + 64 * wn < HW;   // wave-uniform
                v16f pa[2];
                v4f p8[2];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) pa[ni][v] = 0.0f;
                    p8[ni] = v4f{0.f, 0.f, 0.f, 0.f};
                }
                if (live) {
                    v16f acc[2][2];
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        acc[mi][0] = gemm_acc_bias(img + nf7_img_B2(WP) + (2 * wm + mi) * 32 + g * 16);
                        acc[mi][1] = acc[mi][0];
                    }
                    gg_l2<KC, NB>(acc, img + nf7_img_A2(WP) + ((size_t)(2 * wm + 0) * KC * 64 + lane) * 4,
                                  img + nf7_img_A2(WP) + ((size_t)(2 * wm + 1) * KC * 64 + lane) * 4, band + (g * NB + 32 * (2 * wn + 0) + n) * 4,
                                  band + (g * NB + 32 * (2 * wn + 1) + n) * 4);
                    uint32_t gw[2][2];
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            uint16_t *const gp = gate_at(cidx, bnd, 1, (2 * wm + mi) * NT + 2 * wn + ni);
                            if constexpr (RECORD) {
                                gw[mi][ni] = gg_signs(acc[mi][ni]);
                                *gp = (uint16_t)gw[mi][ni];
                            } else {
                                gw[mi][ni] = *gp;
                            }
                        }
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
                        for (int grp = 0; grp < 4; ++grp) {
                            const float4 w0 = ldg4(img + nf7_img_A3(WP) + ((((2 * wm + mi) * 4 + grp) * 64) + lane) * 4);
                            const float4 wc = ldg4(img + nf7_img_A3C(WP) + ((((2 * wm + mi) * 4 + grp) * 8) + g * 4 + (lane & 3)) * 4);
                            const float ws0[4] = {w0.x, w0.y, w0.z, w0.w}, wcs[4] = {wc.x, wc.y, wc.z, wc.w};
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const int v = grp * 4 + s;
                                const float hA = gg_gate(gw[mi][0], v, acc[mi][0][v]), hB = gg_gate(gw[mi][1], v, acc[mi][1][v]);
                                pa[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws0[s], hA, pa[0], 0, 0, 0);
                                pa[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws0[s], hB, pa[1], 0, 0, 0);
                                p8[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(wcs[s], hA, p8[0], 0, 0, 0);
                                p8[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(wcs[s], hB, p8[1], 0, 0, 0);
                            }
                        }
                    }
                }
                __syncthreads();   // every wavefront is done with h1: the region becomes the partial P records

                if (live) {
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) gemm_store_p(band + ((size_t)(wm * NB + 32 * (2 * wn + ni) + n)) * NF7_P_STRIDE, g, pa[ni], p8[ni]);
                }
                __syncthreads();

                // ---- gather: the taps of this band's pixels that fall on the output pixels this thread owns ----
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    const int q = t + GT * m;
                    if (!act[m] || q + W + 1 < p0 || q >= p0 + NB + W + 1) continue;
#pragma unroll
                    for (int di = 0; di < 3; ++di) {
                        const int rr = pr[m] + di - 1;
                        if (rr < 0 || rr >= H) continue;
#pragma unroll
                        for (int dj = 0; dj < 3; ++dj) {
                            const int cc = pc[m] + dj - 1;
                            const int src = rr * W + cc - p0;
                            if (cc < 0 || cc >= W || src < 0 || src >= NB) continue;
#pragma unroll
                            for (int k = 0; k < WM; ++k) {
                                const float *rec = band + ((size_t)(k * NB + src)) * NF7_P_STRIDE;
                                float4 v = *reinterpret_cast<const float4 *>(rec + (di * 3 + dj) * 4);
                                if (di * 3 + dj == 8) {   // tap 8: the two lane halves' partial sums
                                    const float4 u = *reinterpret_cast<const float4 *>(rec + 36);
                                    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
                                }
                                o[m][0] += v.x; o[m][1] += v.y; o[m][2] += v.z; o[m][3] += v.w;
                            }
                        }
                    }
                }
                __syncthreads();   // the next band's l_1 overwrites the region
            }
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                const float4 eb = *reinterpret_cast<const float4 *>(a.params + off + NFGG_CPL_E + 4 * bmask_of(m));
                o[m][0] += eb.x; o[m][1] += eb.y; o[m][2] += eb.z; o[m][3] += eb.w;
            }
        };

        // The three transposed products of a coupling: ga = d nll / d z0 through the CNN, from the d(shift, raw) tile (published and
        // behind a barrier) and the recorded gates.  Ends behind a barrier.
        auto coupling_cnn_t = [&](int off, int cidx, float (&ga)[OWN][2]) {
            const float *const bwd = a.params + off + nfgg_cpl_bwd(WP);
#pragma unroll
            for (int m = 0; m < OWN; ++m) ga[m][0] = ga[m][1] = 0.0f;
            for (int bnd = 0; bnd < n_bands; ++bnd) {
                const int p0 = bnd * NB;
                // ---- l_last^T: 32 tiles of d h2 = gate2(W3 G36), 4 per wavefront, into LDS in B-operand order ----
#pragma unroll 1
                for (int i = 0; i < 4; ++i) {
                    const int tt = wv * 4 + i, m = tt / NT, nt = tt % NT;
                    if (p0 + 32 * nt >= HW) continue;   // wave-uniform
                    int p = p0 + 32 * nt + n;
                    p = p < HW ? p : HW - 1;
                    const int r = p / W, c = p - r * W;
                    // tap (di,dj), element j = 2 (st & 1) + g of d(shift, raw) at pixel - (tap - centre): - di*Wp - dj from here
                    const float *const db = dts + g * PL + (r + 2) * Wp + c + 2;
                    v16f dh;
#pragma unroll
                    for (int v = 0; v < 16; ++v) dh[v] = 0.0f;
#pragma unroll
                    for (int grp = 0; grp < 5; ++grp) {
                        const float4 aw = ldg4(bwd + nfgg_bwd_A3T(WP) + ((m * 5 + grp) * 64 + lane) * 4);
                        const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int st = grp * 4 + s, tap = st >> 1;
                            if (st < 18) dh = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], db[2 * (st & 1) * PL - (tap / 3) * Wp - tap % 3], dh, 0, 0, 0);
                        }
                    }
                    const uint32_t gw = *gate_at(cidx, bnd, 1, tt);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4 *>(band + ((((m * 4 + q) * 2 + g) * NB) + 32 * nt + n) * 4) =
                            make_float4(gg_gate(gw, 4 * q + 0, dh[4 * q + 0]), gg_gate(gw, 4 * q + 1, dh[4 * q + 1]), gg_gate(gw, 4 * q + 2, dh[4 * q + 2]),
                                        gg_gate(gw, 4 * q + 3, dh[4 * q + 3]));
                }
                __syncthreads();

                // ---- l_2^T, gate 1, and D18 = W1 d h1 over this wavefront's 64 channels ----
                const bool live = p0 + 64 * wn < HW;   // wave-uniform
                v16f pd[2];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int v = 0; v < 16; ++v) pd[ni][v] = 0.0f;
                if (live) {
                    v16f acc[2][2];
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.0f;
                    gg_l2<KC, NB>(acc, bwd + nfgg_bwd_A2T(WP) + ((size_t)(2 * wm + 0) * KC * 64 + lane) * 4,
                                  bwd + nfgg_bwd_A2T(WP) + ((size_t)(2 * wm + 1) * KC * 64 + lane) * 4, band + (g * NB + 32 * (2 * wn + 0) + n) * 4,
                                  band + (g * NB + 32 * (2 * wn + 1) + n) * 4);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        const uint32_t gwA = *gate_at(cidx, bnd, 0, (2 * wm + mi) * NT + 2 * wn + 0);
                        const uint32_t gwB = *gate_at(cidx, bnd, 0, (2 * wm + mi) * NT + 2 * wn + 1);
#pragma unroll
                        for (int grp = 0; grp < 4; ++grp) {
                            const float4 w0 = ldg4(bwd + nfgg_bwd_A1T(WP) + ((((2 * wm + mi) * 4 + grp) * 64) + lane) * 4);
                            const float ws0[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const int v = grp * 4 + s;
                                pd[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws0[s], gg_gate(gwA, v, acc[mi][0][v]), pd[0], 0, 0, 0);
                                pd[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws0[s], gg_gate(gwB, v, acc[mi][1][v]), pd[1], 0, 0, 0);
                            }
                        }
                    }
                }
                __syncthreads();   // every wavefront is done with d h2: the region becomes the partial D18 records

                // per pixel [2 tap + ch]: register group aa of lane half g holds rows 8 aa + 4 g .. + 3; rows 0 .. 17 are used
                if (live) {
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        float *dst = band + ((size_t)(wm * NB + 32 * (2 * wn + ni) + n)) * NFGG_D_STRIDE;
#pragma unroll
                        for (int aa = 0; aa < 2; ++aa)
                            *reinterpret_cast<float4 *>(dst + 8 * aa + 4 * g) = make_float4(pd[ni][4 * aa + 0], pd[ni][4 * aa + 1], pd[ni][4 * aa + 2], pd[ni][4 * aa + 3]);
                        if (g == 0) *reinterpret_cast<float4 *>(dst + 16) = make_float4(pd[ni][8], pd[ni][9], pd[ni][10], pd[ni][11]);
                    }
                }
                __syncthreads();

                // ---- scatter as a gather: d z0[q] = sum_taps D18[q - (tap - centre)][tap] over the pixels of this band ----
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    const int q = t + GT * m;
                    if (!act[m] || q + W + 1 < p0 || q >= p0 + NB + W + 1) continue;
#pragma unroll
                    for (int di = 0; di < 3; ++di) {
                        const int rr = pr[m] - (di - 1);
                        if (rr < 0 || rr >= H) continue;
#pragma unroll
                        for (int dj = 0; dj < 3; ++dj) {
                            const int cc = pc[m] - (dj - 1);
                            const int src = rr * W + cc - p0;
                            if (cc < 0 || cc >= W || src < 0 || src >= NB) continue;
#pragma unroll
                            for (int k = 0; k < WM; ++k) {
                                const float2 v = *reinterpret_cast<const float2 *>(band + ((size_t)(k * NB + src)) * NFGG_D_STRIDE + 2 * (di * 3 + dj));
                                ga[m][0] += v.x;
                                ga[m][1] += v.y;
                            }
                        }
                    }
                }
                __syncthreads();   // the next band overwrites the region
            }
        };

        // ---- forward sweep ----
        float z[OWN][4];
        F.load_x(z);
        float ld = 0.0f;
        {
            int cidx = 0;
            for (int op = 0; op < n_ops; ++op) {
                if (prog.ops[op].type != NF_OP_COUPLING_FWD) {
                    F.pointwise_fwd(op, z, ld);
                    continue;
                }
                const cfloat_p P = (cfloat_p)(a.params + prog.ops[op].off);
                float o[OWN][4];
                coupling_cnn(prog.ops[op].off, cidx, std::true_type{}, z, o);
                const float sc = P[NFGG_CPL_S];
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    const float ls0 = sc * nf_tanh(o[m][2]);
                    const float ls1 = sc * nf_tanh(o[m][3]);
                    z[m][2] = fmaf(z[m][2], nf_exp(ls0), o[m][0]);
                    z[m][3] = fmaf(z[m][3], nf_exp(ls1), o[m][1]);
                    if (act[m]) ld += ls0 + ls1;
                }
                ++cidx;
            }
        }
        // nll_b = -(log-det) + prior, as nf_flow_kernel forms it
        if (!TILED && a.nll_out) {
            float s2 = 0.f;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
                if (act[m]) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) s2 = fmaf(z[m][q], z[m][q], s2);
                }
            float r0 = wave_sum(ld), r2 = wave_sum(s2);
            __syncthreads();   // the previous patch's reader is done
            if (lane == 0) {
                red[wv] = r0;
                red[GW + wv] = r2;
            }
            __syncthreads();
            if (t == 0) {
                r0 = 0.f;
                r2 = 0.f;
                for (int k = 0; k < GW; ++k) {
                    r0 += red[k];
                    r2 += red[GW + k];
                }
                const double npx = (double)HW * 4.0;
                const double logdet = (double)r0 + (a.cond_rows ? crow->ld + a.ld_const : a.ld_const);
                a.nll_out[b] = (float)(-logdet + 0.5 * npx * 1.8378770664093453 + 0.5 * (double)r2);
            }
        }

        // ---- backward sweep ----
        float gz[OWN][4];   // d nll / d (the tensor behind the op being undone): the prior's part is z itself
        float gy[OWN][4];
#pragma unroll
        for (int m = 0; m < OWN; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                gz[m][q] = z[m][q];
                gy[m][q] = 0.0f;
            }
        if constexpr (TILED) {
            if (a.g_in) {   // not the last segment: the gradient the segment behind this one stored, whole tile
                const float4 *const g4 = reinterpret_cast<const float4 *>(a.g_in) + patch_off;
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (act[m]) v = g4[gidx_of(m)];
                    gz[m][0] = v.x; gz[m][1] = v.y; gz[m][2] = v.z; gz[m][3] = v.w;
                }
            }
        }
        int cidx = 0;
        for (int op = 0; op < n_ops; ++op) cidx += prog.ops[op].type == NF_OP_COUPLING_FWD ? 1 : 0;
        for (int op = n_ops - 1; op >= 0; --op) {
            const int type = prog.ops[op].type;
            const int off = prog.ops[op].off;
            if (type == NF_OP_COUPLING_FWD) {
                --cidx;
                const cfloat_p P = (cfloat_p)(a.params + off);
                float o[OWN][4];
                coupling_cnn(off, cidx, std::false_type{}, z, o);
                const float sc = P[NFGG_CPL_S];
                // d nll / d (shift, raw) of the owned pixels into the zero-bordered tile (its previous readers passed a barrier)
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    float d[4];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const float th_ = nf_tanh(o[m][2 + q]);
                        const float ls = sc * th_;
                        const float e = nf_exp(ls);
                        const float z1 = (z[m][2 + q] - o[m][q]) * nf_exp(-ls);   // the coupling's input
                        const float dls = fmaf(gz[m][2 + q] * z1, e, -1.0f);
                        d[q] = gz[m][2 + q];
                        d[2 + q] = sc * fmaf(-th_, th_, 1.0f) * dls;
                        gz[m][2 + q] *= e;
                        z[m][2 + q] = z1;
                    }
                    if (act[m]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) dts[j * PL + lidx[m]] = d[j];
                    }
                }
                __syncthreads();
                float ga[OWN][2];
                coupling_cnn_t(off, cidx, ga);
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    gz[m][0] += ga[m][0];
                    gz[m][1] += ga[m][1];
                }
            } else if (type == NF_OP_MIX) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float mm[16], mi[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    mm[i] = P[i];
                    mi[i] = P[16 + i];
                }
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    float zi[4], gi[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float s = z[m][0] * mi[j];
                        s = fmaf(z[m][1], mi[4 + j], s);
                        s = fmaf(z[m][2], mi[8 + j], s);
                        s = fmaf(z[m][3], mi[12 + j], s);
                        zi[j] = s;
                        float q = gz[m][0] * mm[4 * j];
                        q = fmaf(gz[m][1], mm[4 * j + 1], q);
                        q = fmaf(gz[m][2], mm[4 * j + 2], q);
                        q = fmaf(gz[m][3], mm[4 * j + 3], q);
                        gi[j] = q;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        z[m][j] = zi[j];
                        gz[m][j] = gi[j];
                    }
                }
            } else if (type == NF_OP_SDN_DIV) {
                // scale s = sqrt(v), v = a y + b:  z_in = z s,  g_in = g / s,  gy += (a / 2 v) (1 - g_out z_out)
                const float ck1 = F.cond_a(off), cb2 = F.cond_b(off);
                if (op < first_cpl) {   // in front of the first coupling: the op's output, forward from the loaded x
                    float dummy = 0.0f;
                    F.load_x(z);
                    for (int q = 0; q <= op; ++q) F.pointwise_fwd(q, z, dummy);
                }
                float yy[OWN][4];
                F.load_y(yy);
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float v = fmaf(yy[m][q], ck1, cb2);
                        const float r = __builtin_amdgcn_rsqf(v);
                        gy[m][q] = fmaf(0.5f * ck1 * (r * r), fmaf(-gz[m][q], z[m][q], 1.0f), gy[m][q]);
                        gz[m][q] *= r;
                        z[m][q] *= __builtin_amdgcn_sqrtf(v);
                    }
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[0] : F.cond_a(off);
                const float si = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : 1.0f / s;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        gz[m][q] *= s;
                        z[m][q] *= si;
                    }
            }
        }

        if constexpr (TILED) {
            // the core window only; every pixel of the image is in exactly one tile's core, so an accumulating launch adds to gy
            // without atomics (the launch that wrote it is ahead of this one in the stream)
            if (a.g_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.g_out) + patch_off;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
                    if (own_of(m)) o4[gidx_of(m)] = make_float4(gz[m][0], gz[m][1], gz[m][2], gz[m][3]);
            }
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
                const bool acc = (a.tflags & NF_GT_GY_ACC) != 0;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
                    if (own_of(m)) {
                        float4 v = make_float4(gy[m][0], gy[m][1], gy[m][2], gy[m][3]);
                        if (acc) {
                            const float4 p = o4[gidx_of(m)];
                            v = make_float4(p.x + v.x, p.y + v.y, p.z + v.z, p.w + v.w);
                        }
                        o4[gidx_of(m)] = v;
                    }
            }
        } else {
            if (a.gx_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gx_out) + patch_off;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
                    if (act[m]) o4[t + GT * m] = make_float4(gz[m][0], gz[m][1], gz[m][2], gz[m][3]);
            }
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
                    if (act[m]) o4[t + GT * m] = make_float4(gy[m][0], gy[m][1], gy[m][2], gy[m][3]);
            }
        }
    }
}

template <int WP, bool TILED = false>
hipError_t launch_grad_gemm(const NfProgram &prog, const NfGradLaunch &a, int groups, size_t lds, uint16_t *scratch, size_t scratch_halves, hipStream_t stream)
{
    // dynamic LDS beyond 64 KiB is a per-device function attribute: always the CU's whole 160 KiB, set once per device
    static std::atomic<uint32_t> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t bit = 1u << (dev & 31);
    if (!(done.load(std::memory_order_relaxed) & bit) || dev > 31) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&nf_grad_gemm_kernel<WP, TILED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLOW_LDS_MAX);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((nf_grad_gemm_kernel<WP, TILED>), dim3((unsigned)groups), dim3(GT), lds, stream, prog, a, scratch, scratch_halves);
    return hipGetLastError();
}

template <int WP>
hipError_t launch_grad_gemm(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int groups, size_t lds, uint16_t *scratch, size_t scratch_halves,
                            hipStream_t stream)
{
    return tiled ? launch_grad_gemm<WP, true>(prog, a, groups, lds, scratch, scratch_halves, stream)
                 : launch_grad_gemm<WP, false>(prog, a, groups, lds, scratch, scratch_halves, stream);
}

}  // namespace

// the persistent grid of the kernel: one workgroup per CU (the band takes most of a CU's LDS), never more than patches
int nf_grad_gemm_groups(int64_t B, int n_cu)
{
    int64_t groups = n_cu;
    if (B < groups) groups = B;
    return groups < 1 ? 1 : (int)groups;
}

// programs over the GEMM gradient block (nf_gemm_layout.h, NFGG_*).  A tiled segment with more couplings than n_cpl, or a buffer too
// small, is refused before anything is enqueued.
hipError_t nf_launch_grad_gemm(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, void *scratch, size_t scratch_bytes,
                               hipStream_t stream)
{
    static_assert(NF_GRAD_TILE == 32, "a tile is a patch the whole-patch geometry holds");
    const int wp = prog.width;
    if ((wp != 64 && wp != 128 && wp != 256 && wp != 512) || a.H < 1 || a.W < 1 || a.H > 32 || a.W > 32 || n_cpl < 0 || n_cpl > NFGG_MAX_COUPLINGS)
        return hipErrorInvalidValue;
    if (tiled) {
        if (a.H > a.img_H || a.W > a.img_W || a.tile_ny < 1 || a.tile_nx < 1 || a.tile_halo < 0 || !a.z_in) return hipErrorInvalidValue;
        int seg_cpl = 0;
        for (int i = 0; i < prog.n_ops; ++i) seg_cpl += prog.ops[i].type == NF_OP_COUPLING_FWD ? 1 : 0;
        if (seg_cpl > n_cpl) return hipErrorInvalidValue;
    }
    const int groups = nf_grad_gemm_groups(a.B, n_cu);
    const size_t halves = nfgg_gate_halves(a.H * a.W, wp, n_cpl);
    if (halves && (!scratch || scratch_bytes < (size_t)groups * halves * sizeof(uint16_t))) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nfgg_lds_floats(a.H, a.W);
    if (lds > FLOW_LDS_MAX) return hipErrorInvalidValue;
    uint16_t *const s = static_cast<uint16_t *>(scratch);
    switch (wp) {
    case 64: return launch_grad_gemm<64>(prog, a, tiled, groups, lds, s, halves, stream);
    case 128: return launch_grad_gemm<128>(prog, a, tiled, groups, lds, s, halves, stream);
    case 256: return launch_grad_gemm<256>(prog, a, tiled, groups, lds, s, halves, stream);
    default: return launch_grad_gemm<512>(prog, a, tiled, groups, lds, s, halves, stream);
    }
}
