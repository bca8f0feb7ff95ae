// Vector-Jacobian product of sampling at coupling widths 33 .. 512 on the f32 matrix cores of gfx950 (nf_sample_vjp with
// NF_CFG_SVJP_GEMM).
//
// The contract of nf_sample_grad_kernel (nf_sample_grad.hip; its header comment is the specification: sweeps, per-op rules, eps,
// output discipline) in the geometry of nf_grad_gemm_kernel (nf_grad_gemm.hip): one workgroup of 512 threads per patch of up to 32x32
// pixels, grid-stride over patches; thread t owns the pixels t and t + 512 (their z, g and gy live in its registers); the coupling
// CNN at the padded width WP runs BAND by band (NB = 32768 / WP pixels, the band's activations in LDS in B-operand order), weights
// streamed from L2 through the handle's NFGG_* block (nf_gemm_layout.h) — nothing new is uploaded.  The gate record is
// nf_grad_gemm_kernel's: 16 bits per lane and tile, uint16 [coupling][band][layer][tile][lane] in device scratch of THIS WORKGROUP
// (nfgg_gate_halves per workgroup; a workgroup holds one patch at a time), indexed by coupling number, so the sweep order does not
// matter to it.
//   forward sweep   z = eps * temp, then the NLL-order ops LAST TO FIRST, each inverted (nf_sample's arithmetic); a coupling runs the
//                   RECORDING CNN on the pass-through half, then z1 = (z1 - shift) exp(-ls).  x_out stored if asked.
//   backward sweep  g = gx_in, then the ops FIRST TO LAST: every op transforms g (and adds to gy) from its output v, then rebuilds
//                   its input u.  A coupling runs the CNN again on z0 with the RECORDED gates, publishes d(shift, raw) into the
//                   zero-bordered tile and adds the three transposed products' result to g0.  There is no log-det term.
//   end             geps = temp g, gtemp_b = sum over the active pixels of g eps: per thread, wave_sum, then the wavefronts in index
//                   order by thread 0 through `red` — no atomics, the same bits on every run.
// eps — the caller's, or nf_sample's Philox draw zeroed in the slots without a pixel — is regenerated wherever it is needed and never
// held across the sweeps.
// LDS: nfgg_lds_floats(H, W) — the band (128 KiB), the z0 tile (2 planes) and the d(shift, raw) tile (4 planes) at pitch W + 2, the
// reduction scratch: 158 944 B at 32x32, nf_grad_gemm_kernel's budget to the byte (no new LDS).
// Conditioning, loads and the 4x4 product are GradFrame's (nf_grad_common.h).  gg_gate, gg_signs, gg_l2 and the two CNN lambdas
// (coupling_cnn, coupling_cnn_t) are the text of nf_grad_gemm.hip's non-TILED arm: they stand in BOTH files, as GradWide does in
// nf_sample_grad_wide.hip — nf_grad_gemm.hip is not touched, so its instructions stay (profiles/sample_vjp_gemm_asm.txt;
// tests/test_gpu_grad_bits.py pins its bits), and DESIGN 4 ("The rule") keeps such a piece where it is.  A change to one of them is
// made in nf_grad_gemm.hip and here.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <type_traits>

#include "nf_device.h"
#include "nf_gemm_layout.h"
#include "nf_dev_util.h"
#include "nf_internal.h"
#include "nf_gemm_common.h"   // GT, GW, v16f, ldg4, gemm_acc_bias, gemm_store_p
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

// The WP x WP product of a band: this wavefront's 2 x 2 accumulator tiles over the whole K (nf_grad_gemm.hip's gg_l2).
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
//   scratch  the gate records of the launch, `scratch_halves` uint16 per workgroup (nfgg_gate_halves of a.n_cpl couplings)
template <int WP>
__global__ __launch_bounds__(GT) void nf_sample_grad_gemm_kernel(const NfProgram prog, const NfSampleGradLaunch a, uint16_t *const scratch,
                                                                 const size_t scratch_halves)
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
    float *const red = dts + 4 * PL;                 // [GW] of the budgeted [2][GW]

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

    int pr[OWN], pc[OWN], gidx[OWN], lidx[OWN], bmask[OWN];
    bool act[OWN];
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const int p = t + GT * m;
        act[m] = p < HW;
        pr[m] = act[m] ? p / W : 0;
        pc[m] = act[m] ? p - pr[m] * W : 0;
        gidx[m] = act[m] ? p : 0;
        lidx[m] = (pr[m] + 1) * Wp + pc[m] + 1;
        bmask[m] = act[m] ? ((pr[m] == 0 ? 1 : 0) | (pr[m] == H - 1 ? 2 : 0) | (pc[m] == 0 ? 4 : 0) | (pc[m] == W - 1 ? 8 : 0)) : 0;
    }

    const int n_ops = prog.n_ops;
    const int last_cpl = a.last_cpl;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const size_t patch_off = (size_t)b * (size_t)HW;
        const float4 *const y4 = reinterpret_cast<const float4 *>(a.y) + patch_off;   // (not dereferenced when a.y is null)
        const nf_crow_p crow = (nf_crow_p)(a.cond_rows) + b;
        const float4 *const no_in4 = nullptr;   // (the sweep starts from eps: GradFrame::load_x is not used)
        const GradSlotPix<OWN> pix = {act, gidx};
        const GradFrame<OWN, NfSampleGradLaunch, GradSlotPix<OWN>> F = {prog, a, pix, crow, patch_off, no_in4, y4};

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
                const float4 eb = *reinterpret_cast<const float4 *>(a.params + off + NFGG_CPL_E + 4 * bmask[m]);
                o[m][0] += eb.x; o[m][1] += eb.y; o[m][2] += eb.z; o[m][3] += eb.w;
            }
        };

        // The three transposed products of a coupling: ga = d L / d z0 through the CNN, from the d(shift, raw) tile (published and
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

        // eps: the caller's, or nf_sample's draw (the same key), regenerated wherever it is needed
        auto load_eps = [&](float (&e)[OWN][4]) {
            if (a.eps) {
                F.load4(a.eps, 0.0f, e);
            } else {
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    philox_normal4(a.seed, a.patch_base + b, (uint32_t)gidx[m], NF_STREAM_SAMP, e[m]);
                    if (!act[m]) e[m][0] = e[m][1] = e[m][2] = e[m][3] = 0.0f;
                }
            }
        };
        // the pointwise ops in the sampling direction (nf_sample's arithmetic): the inverse of NLL-order op `op`
        auto pointwise_inv = [&](int op, float (&z)[OWN][4]) {
            const int type = prog.ops[op].type;
            const int off = prog.ops[op].off;
            if (type == NF_OP_MIX) {
                F.mat4((cfloat_p)(a.params + off) + 16, z);
            } else if (type == NF_OP_SDN_DIV) {
                const float ck1 = F.cond_a(off), cb2 = F.cond_b(off);
                float yy[OWN][4];
                F.load_y(yy);
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[m][q] *= __builtin_amdgcn_sqrtf(fmaf(yy[m][q], ck1, cb2));
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : F.cond_a(off);
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[m][q] *= s;
            }
        };

        // ---- forward sweep: x = f(y, eps, temp) ----
        float z[OWN][4];
        load_eps(z);
#pragma unroll
        for (int m = 0; m < OWN; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) z[m][q] *= a.temp;
        {
            int cidx = a.n_cpl;
            for (int op = n_ops - 1; op >= 0; --op) {
                if (prog.ops[op].type != NF_OP_COUPLING_FWD) {
                    pointwise_inv(op, z);
                    continue;
                }
                --cidx;
                const cfloat_p P = (cfloat_p)(a.params + prog.ops[op].off);
                float o[OWN][4];
                coupling_cnn(prog.ops[op].off, cidx, std::true_type{}, z, o);
                const float sc = P[NFGG_CPL_S];
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    const float ls0 = sc * nf_tanh(o[m][2]);
                    const float ls1 = sc * nf_tanh(o[m][3]);
                    z[m][2] = (z[m][2] - o[m][0]) * nf_exp(-ls0);
                    z[m][3] = (z[m][3] - o[m][1]) * nf_exp(-ls1);
                }
            }
        }
        if (a.x_out) {
            float4 *const o4 = reinterpret_cast<float4 *>(a.x_out) + patch_off;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
                if (act[m]) o4[gidx[m]] = make_float4(z[m][0], z[m][1], z[m][2], z[m][3]);
        }

        // ---- backward sweep ----
        float gz[OWN][4];   // d L / d (the tensor in front of the NLL-order op being reached): gx_in at the start
        float gy[OWN][4];
        F.load4(a.gx_in, 0.0f, gz);
#pragma unroll
        for (int m = 0; m < OWN; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) gy[m][q] = 0.0f;
        int cidx = 0;
        for (int op = 0; op < n_ops; ++op) {
            const int type = prog.ops[op].type;
            const int off = prog.ops[op].off;
            if (type == NF_OP_COUPLING_FWD) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float o[OWN][4];
                coupling_cnn(off, cidx, std::false_type{}, z, o);
                const float sc = P[NFGG_CPL_S];
                // d L / d (shift, raw) of the owned pixels into the zero-bordered tile (its previous readers passed a barrier)
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    float d[4];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const float th_ = nf_tanh(o[m][2 + q]);
                        const float ls = sc * th_;
                        const float gu = gz[m][2 + q] * nf_exp(-ls);
                        const float dls = -gz[m][2 + q] * z[m][2 + q];
                        d[q] = -gu;
                        d[2 + q] = sc * fmaf(-th_, th_, 1.0f) * dls;
                        gz[m][2 + q] = gu;
                        z[m][2 + q] = fmaf(z[m][2 + q], nf_exp(ls), o[m][q]);   // the sampling op's input
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
                ++cidx;
            } else if (type == NF_OP_MIX) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float mi[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) mi[i] = P[16 + i];
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    float gi[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {   // g Ainv^T
                        float q = gz[m][0] * mi[4 * j];
                        q = fmaf(gz[m][1], mi[4 * j + 1], q);
                        q = fmaf(gz[m][2], mi[4 * j + 2], q);
                        q = fmaf(gz[m][3], mi[4 * j + 3], q);
                        gi[j] = q;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) gz[m][j] = gi[j];
                }
                F.mat4(P, z);   // u = v A
            } else if (type == NF_OP_SDN_DIV) {
                const float ck1 = F.cond_a(off), cb2 = F.cond_b(off);
                if (op > last_cpl) {   // the first ops sampling runs: the op's output, forward from eps * temp
                    load_eps(z);
#pragma unroll
                    for (int m = 0; m < OWN; ++m)
#pragma unroll
                        for (int q = 0; q < 4; ++q) z[m][q] *= a.temp;
                    for (int q = n_ops - 1; q >= op; --q) pointwise_inv(q, z);
                }
                float yy[OWN][4];
                F.load_y(yy);
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float v = fmaf(yy[m][q], ck1, cb2);
                        const float r = __builtin_amdgcn_rsqf(v);
                        gy[m][q] = fmaf(0.5f * ck1 * (r * r), gz[m][q] * z[m][q], gy[m][q]);
                        gz[m][q] *= __builtin_amdgcn_sqrtf(v);
                        z[m][q] *= r;
                    }
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : F.cond_a(off);
                const float si = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[0] : 1.0f / s;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        gz[m][q] *= s;
                        z[m][q] *= si;
                    }
            }
        }

        if (a.gy_out) {
            float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
                if (act[m]) o4[gidx[m]] = make_float4(gy[m][0], gy[m][1], gy[m][2], gy[m][3]);
        }
        if (a.geps_out) {
            float4 *const o4 = reinterpret_cast<float4 *>(a.geps_out) + patch_off;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
                if (act[m]) o4[gidx[m]] = make_float4(a.temp * gz[m][0], a.temp * gz[m][1], a.temp * gz[m][2], a.temp * gz[m][3]);
        }
        if (a.gtemp_out) {   // wave-uniform
            load_eps(z);
            float s = 0.0f;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q) s = act[m] ? fmaf(gz[m][q], z[m][q], s) : s;
            float r = wave_sum(s);
            __syncthreads();   // the previous patch's reader is done
            if (lane == 0) red[wv] = r;
            __syncthreads();
            if (t == 0) {
                r = 0.f;
                for (int k = 0; k < GW; ++k) r += red[k];
                a.gtemp_out[b] = r;
            }
        }
    }
}

template <int WP>
hipError_t launch_sgrad_gemm(const NfProgram &prog, const NfSampleGradLaunch &a, int groups, size_t lds, uint16_t *scratch, size_t scratch_halves,
                             hipStream_t stream)
{
    // dynamic LDS beyond 64 KiB is a per-device function attribute: always the CU's whole 160 KiB, set once per device
    static std::atomic<uint32_t> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint32_t bit = 1u << (dev & 31);
    if (!(done.load(std::memory_order_relaxed) & bit) || dev > 31) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&nf_sample_grad_gemm_kernel<WP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLOW_LDS_MAX);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((nf_sample_grad_gemm_kernel<WP>), dim3((unsigned)groups), dim3(GT), lds, stream, prog, a, scratch, scratch_halves);
    return hipGetLastError();
}

}  // namespace

// entry point used by nf_host.hip (which has checked the supported set: sample_vjp_support); programs over the GEMM gradient block
// (nf_gemm_layout.h, NFGG_*).  The grid and the size the scratch is held to come from the one function, nf_grad_gemm_groups, and the
// record's couplings from the program itself: a buffer too small, or an a.n_cpl that is not the program's, is refused before anything
// is enqueued.
hipError_t nf_launch_sample_grad_gemm(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, void *scratch, size_t scratch_bytes, hipStream_t stream)
{
    const int wp = prog.width;
    if ((wp != 64 && wp != 128 && wp != 256 && wp != 512) || a.H < 1 || a.W < 1 || a.H > 32 || a.W > 32 || a.B < 1) return hipErrorInvalidValue;
    int n_cpl = 0;
    for (int i = 0; i < prog.n_ops; ++i) n_cpl += prog.ops[i].type == NF_OP_COUPLING_FWD ? 1 : 0;
    if (n_cpl != a.n_cpl || n_cpl > NFGG_MAX_COUPLINGS) return hipErrorInvalidValue;
    const int groups = nf_grad_gemm_groups(a.B, n_cu);
    const size_t halves = nfgg_gate_halves(a.H * a.W, wp, n_cpl);
    if (halves && (!scratch || scratch_bytes < (size_t)groups * halves * sizeof(uint16_t))) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nfgg_lds_floats(a.H, a.W);
    if (lds > FLOW_LDS_MAX) return hipErrorInvalidValue;
    uint16_t *const s = static_cast<uint16_t *>(scratch);
    switch (wp) {
    case 64: return launch_sgrad_gemm<64>(prog, a, groups, lds, s, halves, stream);
    case 128: return launch_sgrad_gemm<128>(prog, a, groups, lds, s, halves, stream);
    case 256: return launch_sgrad_gemm<256>(prog, a, groups, lds, s, halves, stream);
    default: return launch_sgrad_gemm<512>(prog, a, groups, lds, s, halves, stream);
    }
}
