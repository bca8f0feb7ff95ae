// Vector-Jacobian product of sampling (nf_sample_vjp): given g = d L / d x of x = sample(y, eps, temp), one fused kernel returns
// d L / d y, d L / d eps and d L / d temp (per patch) — and x itself, if asked.
//
// The design is nf_grad_kernel's (nf_grad.hip) run in the other direction: one workgroup per patch, grid-stride over patches, the
// handle's scalar gradient block with scalar (SGPR) weights, the same pixel slots (nf_grad_threads, nf_grad_px; one exception:
// width 8 beyond 1 024 pixels, dispatch_sgrad below), the same two zero-bordered LDS tiles, gate record (nf_grad_gate_words) and
// LDS budget (nf_grad_lds_floats).  Per patch:
//   forward sweep   z = eps * temp (the caller's eps or nf_sample's Philox draw), then the NLL-order ops LAST TO FIRST, each inverted
//                   (nf_sample's arithmetic): x — and every ReLU gate recorded as one bit;
//   backward sweep  g = gx_in, then the ops FIRST TO LAST.  With v the output of an op's inverse and u its input, every op first
//                   transforms g (and adds to gy) from v, then rebuilds u — the NLL-direction op applied to v: no activation is
//                   stored, HBM traffic is y, eps, g in and the gradients out.
//     MIX       v = u Ainv            g <- g Ainv^T                                     u = v A
//     COUPLING  v1 = (u1 - shift(u0)) exp(-ls(u0)), ls = S tanh(raw)
//               d shift = -g1 exp(-ls), d ls = -g1 v1, d raw = S (1 - tanh^2) d ls, g1 <- g1 exp(-ls),
//               g0 <- g0 + CNN^T(d shift, d raw) through the RECORDED gates         u1 = v1 exp(ls) + shift
//     SDN       v = u s, s^2 = a y + b   gy += g v a / (2 s^2), g <- g s                 u = v / s
//     SCALE     v = u c                  g <- g c                                        u = v / c
//   end             geps = temp g, gtemp_b = sum over the patch of g eps (per thread, wavefront, then the wavefronts in order: no
//                   atomics, the same bits on every run).
// The gates come from the forward sweep, not from the rebuilt values: the result is the derivative of the function the forward
// sweep evaluated.  The ops behind the last coupling in NLL order (the first ones sampling runs) take their values forward from
// eps * temp instead of the rebuilt ones, as nf_grad_kernel does for the ops behind x.
// The frame (conditioning, loads, the 4x4 product) and the gate record with the coupling CNN are nf_grad_common.h's, shared with
// nf_grad_kernel; slot set-up and the transposed pass stand inline in both kernels (nf_grad_common.h says why).
//
// TILED (NF_CFG_SVJP_TILED, nf_device.h "gradient tiles", NfSampleGradTileLaunch): a "patch" of the launch is one H x W tile of an
// img_H x img_W image and `prog` one SEGMENT of the NLL-order program.  The tile starts from the tensor kept at the segment's
// sampling-side input (z_in; the NLL-last segment from eps * temp, the draw keyed by image and image pixel), runs the same forward
// sweep over the segment's ops, takes g from g_in (the caller's gx_in, or what the segment in front of it stored), runs the same
// backward sweep and stores its CORE window only: g_out, or (NLL-last) geps_out = temp g and the tile's sum of g eps over its core
// (tile_sum; nf_tile_sum_kernel adds an image's tiles up in tile order); gy_out stored or added to.  Border masks follow the image
// border, conditioning rows are per image, and x is not formed here (the tiled nf_sample launches in front of this one form it).
// The whole-patch instantiations keep the parent's instructions (profiles/sample_vjp_tiled_asm.txt): what TILED changes stands in
// `if constexpr` arms, and its fields in a launch record of its own.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <type_traits>

#include "nf_device.h"
#include "nf_dev_util.h"
#include "nf_internal.h"
#include "nf_flow_common.h"   // flow_launch: the persistent-grid launcher
#include "nf_grad_common.h"   // GradFrame, GradCoupling

namespace {

// the launch record: a tiled launch's carries the tile / image fields behind the whole-patch record (nf_device.h)
template <bool TILED>
using SGradArgs = std::conditional_t<TILED, NfSampleGradTileLaunch, NfSampleGradLaunch>;

template <int WIDTH, int THREADS, int PX, bool TILED = false>
__global__ __launch_bounds__(THREADS) void nf_sample_grad_kernel(const NfProgram prog, const SGradArgs<TILED> a)
{
    using ARGS = SGradArgs<TILED>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NPIX = THREADS * PX;
    constexpr int NW = THREADS / 64;
    const int H = a.H, W = a.W, HW = H * W, Wp = W + 2;
    const int tile_px = ((H + 2) * Wp + 1) & ~1;
    float2 *const t0 = reinterpret_cast<float2 *>(smem);   // z0 tile [tile_px] float2
    float *const th = smem + 2 * tile_px;                   // relu(h2) / d(shift, raw) / d h1 tile [tile_px][WIDTH]
    uint32_t *const gates = reinterpret_cast<uint32_t *>(th + (size_t)tile_px * WIDTH);   // [gate_words][NPIX]
    float *const red = reinterpret_cast<float *>(gates + (size_t)a.gate_words * NPIX);    // [NW]

    const int t = threadIdx.x;
    int lidx[PX], gidx[PX], bmask[PX];
    bool act[PX];
    [[maybe_unused]] int prow[PX], pcol[PX];   // TILED: row / column of the slot's pixel inside the tile
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int p = t + THREADS * k;
        act[k] = p < HW;
        const int pp = act[k] ? p : 0;
        const int r = pp / W, c = pp - r * W;
        gidx[k] = pp;
        prow[k] = r;
        pcol[k] = c;
        lidx[k] = (r + 1) * Wp + (c + 1);
        bmask[k] = (r == 0 ? 1 : 0) | (r == H - 1 ? 2 : 0) | (c == 0 ? 4 : 0) | (c == W - 1 ? 8 : 0);
    }
    // zero both tiles once: the 1-pixel border is never written again
    for (int i = t; i < tile_px * (2 + WIDTH); i += THREADS) smem[i] = 0.0f;
    __syncthreads();

    const int n_ops = prog.n_ops;
    const int last_cpl = a.last_cpl;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        // Where this "patch" sits: on its own, or — TILED — as tile b % tiles of image b / tiles (nf_device.h, "overlapping tiles"):
        // addresses, border masks and the Philox key follow the image, own[] is the tile's core window
        int64_t img = b;
        [[maybe_unused]] bool own[PX];
        if constexpr (TILED) {
            const int nt = a.tile_ny * a.tile_nx;
            img = b / nt;
            const int ti = (int)(b - img * nt);
            const int ty = ti / a.tile_nx, tx = ti - ty * a.tile_nx;
            const int oy = nf_tile_origin(ty, a.img_H, H, a.tile_halo), ox = nf_tile_origin(tx, a.img_W, W, a.tile_halo);
            const int cy0 = nf_tile_core0(ty, a.img_H, H, a.tile_halo), cy1 = nf_tile_core1(ty, a.tile_ny, a.img_H, H, a.tile_halo);
            const int cx0 = nf_tile_core0(tx, a.img_W, W, a.tile_halo), cx1 = nf_tile_core1(tx, a.tile_nx, a.img_W, W, a.tile_halo);
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const int R = oy + prow[k], C = ox + pcol[k];
                gidx[k] = R * a.img_W + C;
                bmask[k] = (R == 0 ? 1 : 0) | (R == a.img_H - 1 ? 2 : 0) | (C == 0 ? 4 : 0) | (C == a.img_W - 1 ? 8 : 0);
                own[k] = act[k] && R >= cy0 && R < cy1 && C >= cx0 && C < cx1;
            }
        }
        const size_t patch_off = [&] {
            if constexpr (TILED) return (size_t)img * (size_t)a.img_H * (size_t)a.img_W;
            else return (size_t)b * (size_t)HW;
        }();
        const float4 *const y4 = reinterpret_cast<const float4 *>(a.y) + patch_off;   // (not dereferenced when a.y is null)
        const nf_crow_p crow = (nf_crow_p)(a.cond_rows) + img;
        const float4 *const no_in4 = nullptr;   // (the sweep starts from eps: GradFrame::load_x is not used)
        const GradSlotPix<PX> pix = {act, gidx};
        const GradFrame<PX, ARGS, GradSlotPix<PX>> F = {prog, a, pix, crow, patch_off, no_in4, y4};
        // the sampling sweep reaches the couplings LAST TO FIRST: GradCoupling's LAST_FIRST numbering of the gate sets
        const GradCoupling<WIDTH, THREADS, PX, ARGS, true> cpl = {a, act, t0, lidx, Wp, gates, t, th, bmask};

        // eps: the caller's, or nf_sample's draw (the same key), regenerated wherever it is needed
        auto load_eps = [&](float (&e)[PX][4]) {
            if (a.eps) {
                F.load4(a.eps, 0.0f, e);
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    philox_normal4(a.seed, a.patch_base + img, (uint32_t)gidx[k], NF_STREAM_SAMP, e[k]);
                    if (!act[k]) e[k][0] = e[k][1] = e[k][2] = e[k][3] = 0.0f;
                }
            }
        };
        // the pointwise ops in the sampling direction (nf_sample's arithmetic): the inverse of NLL-order op `op`
        auto pointwise_inv = [&](int op, float (&z)[PX][4]) {
            const int type = prog.ops[op].type;
            const int off = prog.ops[op].off;
            if (type == NF_OP_MIX) {
                F.mat4((cfloat_p)(a.params + off) + 16, z);
            } else if (type == NF_OP_SDN_DIV) {
                const float ck1 = F.cond_a(off), cb2 = F.cond_b(off);
                float yy[PX][4];
                F.load_y(yy);
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) z[k][c] *= __builtin_amdgcn_sqrtf(fmaf(yy[k][c], ck1, cb2));
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : F.cond_a(off);
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) z[k][c] *= s;
            }
        };

        // the tensor the sweep starts from: eps * temp — TILED: or the tensor kept at the segment's sampling-side input
        auto load_start = [&](float (&v)[PX][4]) {
            if constexpr (TILED) {
                if (a.z_in) {
                    F.load4(a.z_in, 0.0f, v);
                    return;
                }
            }
            load_eps(v);
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) v[k][c] *= a.temp;
        };

        // ---- forward sweep: x = f(y, eps, temp) ----
        float z[PX][4];
        if constexpr (TILED) {
            load_start(z);
        } else {
            load_eps(z);
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) z[k][c] *= a.temp;
        }
        {
            int cidx = a.n_cpl;
            for (int op = n_ops - 1; op >= 0; --op) {
                if (prog.ops[op].type != NF_OP_COUPLING_FWD) {
                    pointwise_inv(op, z);
                    continue;
                }
                --cidx;
                const cfloat_p P = (cfloat_p)(a.params + prog.ops[op].off);
                float o[PX][4];
                cpl.template cnn<true>(prog.ops[op].off, cidx, z, o);
                const float sc = P[nf_cpl_off_S(WIDTH)];
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const float ls0 = sc * nf_tanh(o[k][2]);
                    const float ls1 = sc * nf_tanh(o[k][3]);
                    z[k][2] = (z[k][2] - o[k][0]) * nf_exp(-ls0);
                    z[k][3] = (z[k][3] - o[k][1]) * nf_exp(-ls1);
                }
            }
        }
        if (!TILED && a.x_out) {   // (TILED: the tiled nf_sample launches in front of this one form x)
            float4 *const o4 = reinterpret_cast<float4 *>(a.x_out) + patch_off;
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (act[k]) o4[gidx[k]] = make_float4(z[k][0], z[k][1], z[k][2], z[k][3]);
        }

        // ---- backward sweep ----
        float g[PX][4];    // d L / d (the tensor in front of the NLL-order op being reached): gx_in at the start
        float gy[PX][4];
        if constexpr (TILED) F.load4(a.g_in, 0.0f, g);
        else F.load4(a.gx_in, 0.0f, g);
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) gy[k][c] = 0.0f;
        int cidx = 0;
        for (int op = 0; op < n_ops; ++op) {
            const int type = prog.ops[op].type;
            const int off = prog.ops[op].off;
            if (type == NF_OP_COUPLING_FWD) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float o[PX][4];
                cpl.template cnn<false>(off, cidx, z, o);
                const float sc = P[nf_cpl_off_S(WIDTH)];
                float d[PX][4];   // d L / d (shift, raw)
#pragma unroll
                for (int k = 0; k < PX; ++k) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const float th_ = nf_tanh(o[k][2 + c]);
                        const float ls = sc * th_;
                        const float gu = g[k][2 + c] * nf_exp(-ls);
                        const float dls = -g[k][2 + c] * z[k][2 + c];
                        d[k][c] = -gu;
                        d[k][2 + c] = sc * fmaf(-th_, th_, 1.0f) * dls;
                        g[k][2 + c] = gu;
                        z[k][2 + c] = fmaf(z[k][2 + c], nf_exp(ls), o[k][c]);   // the sampling op's input
                    }
                }
                __syncthreads();   // relu(h2) consumed: d(shift, raw) overlays it
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) *reinterpret_cast<float4 *>(th + (size_t)lidx[k] * WIDTH) = make_float4(d[k][0], d[k][1], d[k][2], d[k][3]);
                __syncthreads();
                // W3^T over the zero-bordered tile: d relu(h2)[q][i] = sum_taps sum_j d[q - tap][j] W3[tap][i][j]
                float dh[PX][WIDTH];
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int i = 0; i < WIDTH; ++i) dh[k][i] = 0.0f;
                {
                    const cfloat_p W3 = P + nf_cpl_off_W3(WIDTH);
#pragma unroll 1
                    for (int di = 0; di < 3; ++di) {
                        const cfloat_p W3r = W3 + di * (3 * WIDTH * 4);
                        const int roff = -(di - 1) * Wp + 1;
#pragma unroll
                        for (int dj = 0; dj < 3; ++dj) {
#pragma unroll
                            for (int k = 0; k < PX; ++k) {
                                const float4 dv = *reinterpret_cast<const float4 *>(th + (size_t)(lidx[k] + roff - dj) * WIDTH);
                                const float dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                                for (int i = 0; i < WIDTH; ++i)
#pragma unroll
                                    for (int j = 0; j < 4; ++j) dh[k][i] = fmaf(dd[j], W3r[(dj * WIDTH + i) * 4 + j], dh[k][i]);
                            }
                        }
                    }
                }
                // through the recorded gates and W2^T: d h1
                {
                    const cfloat_p W2 = P + nf_cpl_off_W2(WIDTH);
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int gs = 2 * (a.n_cpl - 1 - cidx);
                        const uint32_t g1 = cpl.gate_get(gs, k), g2 = cpl.gate_get(gs + 1, k);
                        float d2[WIDTH];
#pragma unroll
                        for (int j = 0; j < WIDTH; ++j) d2[j] = ((g2 >> j) & 1u) ? dh[k][j] : 0.0f;
#pragma unroll
                        for (int i = 0; i < WIDTH; ++i) {
                            float s = 0.0f;
#pragma unroll
                            for (int j = 0; j < WIDTH; ++j) s = fmaf(d2[j], W2[i * WIDTH + j], s);
                            dh[k][i] = ((g1 >> i) & 1u) ? s : 0.0f;
                        }
                    }
                }
                __syncthreads();   // d(shift, raw) consumed: d h1 overlays it
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) {
                        float4 *const dst = reinterpret_cast<float4 *>(th + (size_t)lidx[k] * WIDTH);
#pragma unroll
                        for (int q = 0; q < WIDTH / 4; ++q) dst[q] = make_float4(dh[k][4 * q], dh[k][4 * q + 1], dh[k][4 * q + 2], dh[k][4 * q + 3]);
                    }
                __syncthreads();
                // W1^T over the zero-bordered tile, added to the pass-through half's gradient
                {
                    const cfloat_p W1 = P + nf_cpl_off_W1(WIDTH);
#pragma unroll 1
                    for (int di = 0; di < 3; ++di) {
                        const cfloat_p W1r = W1 + di * (3 * 2 * WIDTH);
                        const int roff = -(di - 1) * Wp + 1;
#pragma unroll
                        for (int dj = 0; dj < 3; ++dj) {
#pragma unroll
                            for (int q = 0; q < WIDTH / 4; ++q) {
#pragma unroll
                                for (int k = 0; k < PX; ++k) {
                                    const float4 hv = *reinterpret_cast<const float4 *>(th + (size_t)(lidx[k] + roff - dj) * WIDTH + 4 * q);
                                    const float hh[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                                    for (int i = 0; i < 4; ++i) {
                                        g[k][0] = fmaf(hh[i], W1r[(dj * 2 + 0) * WIDTH + 4 * q + i], g[k][0]);
                                        g[k][1] = fmaf(hh[i], W1r[(dj * 2 + 1) * WIDTH + 4 * q + i], g[k][1]);
                                    }
                                }
                            }
                        }
                    }
                }
                ++cidx;
            } else if (type == NF_OP_MIX) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float mi[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) mi[i] = P[16 + i];
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    float gi[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {   // g Ainv^T
                        float q = g[k][0] * mi[4 * j];
                        q = fmaf(g[k][1], mi[4 * j + 1], q);
                        q = fmaf(g[k][2], mi[4 * j + 2], q);
                        q = fmaf(g[k][3], mi[4 * j + 3], q);
                        gi[j] = q;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) g[k][j] = gi[j];
                }
                F.mat4(P, z);   // u = v A
            } else if (type == NF_OP_SDN_DIV) {
                const float ck1 = F.cond_a(off), cb2 = F.cond_b(off);
                if (op > last_cpl) {   // the first ops sampling runs: the op's output, forward from eps * temp
                    if constexpr (TILED) {
                        load_start(z);
                    } else {
                        load_eps(z);
#pragma unroll
                        for (int k = 0; k < PX; ++k)
#pragma unroll
                            for (int c = 0; c < 4; ++c) z[k][c] *= a.temp;
                    }
                    for (int q = n_ops - 1; q >= op; --q) pointwise_inv(q, z);
                }
                float yy[PX][4];
                F.load_y(yy);
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float v = fmaf(yy[k][c], ck1, cb2);
                        const float r = __builtin_amdgcn_rsqf(v);
                        gy[k][c] = fmaf(0.5f * ck1 * (r * r), g[k][c] * z[k][c], gy[k][c]);
                        g[k][c] *= __builtin_amdgcn_sqrtf(v);
                        z[k][c] *= r;
                    }
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : F.cond_a(off);
                const float si = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[0] : 1.0f / s;
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        g[k][c] *= s;
                        z[k][c] *= si;
                    }
            }
        }

        if constexpr (TILED) {
            // the core window only; every pixel of the image is in exactly one tile's core, so an accumulating launch adds to gy
            // without atomics (the launch that wrote it is ahead of this one in the stream)
            if (a.g_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.g_out) + patch_off;
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (own[k]) o4[gidx[k]] = make_float4(g[k][0], g[k][1], g[k][2], g[k][3]);
            }
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
                const bool acc = (a.tflags & NF_GT_GY_ACC) != 0;
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (own[k]) {
                        float4 v = make_float4(gy[k][0], gy[k][1], gy[k][2], gy[k][3]);
                        if (acc) {
                            const float4 p = o4[gidx[k]];
                            v = make_float4(p.x + v.x, p.y + v.y, p.z + v.z, p.w + v.w);
                        }
                        o4[gidx[k]] = v;
                    }
            }
            if (a.geps_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.geps_out) + patch_off;
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (own[k]) o4[gidx[k]] = make_float4(a.temp * g[k][0], a.temp * g[k][1], a.temp * g[k][2], a.temp * g[k][3]);
            }
            if (a.tile_sum) {   // wave-uniform: the tile's share of gtemp, its core only
                load_eps(z);
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) s = own[k] ? fmaf(g[k][c], z[k][c], s) : s;
                float r = wave_sum(s);
                if constexpr (NW > 1) {
                    __syncthreads();   // the previous tile's reader is done
                    if ((t & 63) == 0) red[t >> 6] = r;
                    __syncthreads();
                    if (t == 0) {
                        r = 0.f;
                        for (int wv = 0; wv < NW; ++wv) r += red[wv];
                    }
                }
                if (t == 0) a.tile_sum[b] = r;
            }
        } else {
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
    #pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) o4[gidx[k]] = make_float4(gy[k][0], gy[k][1], gy[k][2], gy[k][3]);
            }
            if (a.geps_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.geps_out) + patch_off;
    #pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) o4[gidx[k]] = make_float4(a.temp * g[k][0], a.temp * g[k][1], a.temp * g[k][2], a.temp * g[k][3]);
            }
            if (a.gtemp_out) {   // wave-uniform
                load_eps(z);
                float s = 0.0f;
    #pragma unroll
                for (int k = 0; k < PX; ++k)
    #pragma unroll
                    for (int c = 0; c < 4; ++c) s = act[k] ? fmaf(g[k][c], z[k][c], s) : s;
                float r = wave_sum(s);
                if constexpr (NW > 1) {
                    __syncthreads();   // the previous patch's reader is done
                    if ((t & 63) == 0) red[t >> 6] = r;
                    __syncthreads();
                    if (t == 0) {
                        r = 0.f;
                        for (int wv = 0; wv < NW; ++wv) r += red[wv];
                    }
                }
                if (t == 0) a.gtemp_out[b] = r;
            }
        }
    }
}

template <int WIDTH, int THREADS, int PX, bool TILED = false>
hipError_t launch_sgrad(const NfProgram &prog, const SGradArgs<TILED> &a, int n_cu, size_t lds, hipStream_t stream)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return flow_launch<&nf_sample_grad_kernel<WIDTH, THREADS, PX, TILED>>(THREADS, lds, prog, a, n_cu, dev, stream);
}

// the geometries of nf_grad.hip's dispatch_grad (nf_grad_threads, nf_grad_px), but for width 8 beyond 1 024 pixels: 768 x 4 pixel slots,
// fewer than nf_grad_lds_floats budgets the gate record for (the kernel sizes its record by ITS slots: the budget is never exceeded)
template <int WIDTH>
hipError_t dispatch_sgrad(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    const int hw = a.H * a.W;
    if (hw <= 64) return launch_sgrad<WIDTH, 64, 1>(prog, a, n_cu, lds, stream);
    if (hw <= 256) return launch_sgrad<WIDTH, 256, 1>(prog, a, n_cu, lds, stream);
    if constexpr (WIDTH >= 32) {
        if (hw <= 1024) return launch_sgrad<WIDTH, 1024, 1>(prog, a, n_cu, lds, stream);
    } else {
        if (hw <= 1024) return launch_sgrad<WIDTH, 256, 4>(prog, a, n_cu, lds, stream);
        // beyond 1 024 pixels a lane holds 4 pixels.  Width 4 does inside the 128 VGPRs of a 1 024-thread workgroup (155 spilled);
        // width 8 runs 768 threads (168 VGPRs: up to 3 072 pixels, nearly all that the LDS budget leaves it) — its 1 024-thread
        // build returned wrong gradients on the GPU and is not instantiated
        if constexpr (WIDTH == 4) {
            if (hw <= 4096) return launch_sgrad<WIDTH, 1024, 4>(prog, a, n_cu, lds, stream);
        } else if constexpr (WIDTH == 8) {
            if (hw <= NF_SVJP_W8_MAX_PIXELS) return launch_sgrad<WIDTH, 768, 4>(prog, a, n_cu, lds, stream);
        }
    }
    return hipErrorInvalidValue;
}

// TILED: tiles are at most 32x32 (nf_device.h, NF_GRAD_TILE) — the three geometries nf_grad.hip tiles with, widths 4 / 8 / 16 (no
// 1 024-thread or 768-thread build, and none at width 32)
template <int WIDTH>
hipError_t dispatch_sgrad_tiled(const NfProgram &prog, const NfSampleGradTileLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    const int hw = a.H * a.W;
    if (hw <= 64) return launch_sgrad<WIDTH, 64, 1, true>(prog, a, n_cu, lds, stream);
    if (hw <= 256) return launch_sgrad<WIDTH, 256, 1, true>(prog, a, n_cu, lds, stream);
    if (hw <= 1024) return launch_sgrad<WIDTH, 256, 4, true>(prog, a, n_cu, lds, stream);
    return hipErrorInvalidValue;
}

// gtemp of a tiled call: image b's tile sums (what the NLL-last segment's launch left, [image][tile]) added in tile order by one
// thread — no atomics, the same bits on every run
__global__ __launch_bounds__(64) void nf_tile_sum_kernel(const float *__restrict__ part, int nt, int64_t B, float *__restrict__ out)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *const p = part + b * nt;
    float s = 0.0f;
    for (int i = 0; i < nt; ++i) s += p[i];
    out[b] = s;
}

}  // namespace

hipError_t nf_launch_tile_sum(const float *part, int nt, int64_t B, float *out, hipStream_t stream)
{
    if (!part || !out || nt < 1 || B < 1 || (B + 63) / 64 > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nf_tile_sum_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, part, nt, B, out);
    return hipGetLastError();
}

// entry points used by nf_host.hip (which has checked the supported set: sample_vjp_support): whole patches ...
hipError_t nf_launch_sample_grad(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, hipStream_t stream)
{
    if (a.H < 1 || a.W < 1 || a.H > 64 || a.W > 64) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nf_grad_lds_floats(a.H, a.W, prog.width, a.n_cpl);
    if (lds > 160 * 1024 || a.gate_words != nf_grad_gate_words(a.n_cpl, prog.width)) return hipErrorInvalidValue;
    switch (prog.width) {
    case 4: return dispatch_sgrad<4>(prog, a, n_cu, lds, stream);
    case 8: return dispatch_sgrad<8>(prog, a, n_cu, lds, stream);
    case 16: return dispatch_sgrad<16>(prog, a, n_cu, lds, stream);
    case 32: return dispatch_sgrad<32>(prog, a, n_cu, lds, stream);
    default: return hipErrorInvalidValue;
    }
}

// ... and one segment of a tiled call: `prog` = the segment's ops, a.H x a.W = the tile, a.B = images x tiles, n_cpl = the couplings
// of the call's largest segment (what a.gate_words and the LDS are sized by; a.n_cpl = the segment's own)
hipError_t nf_launch_sample_grad_tiled(const NfProgram &prog, const NfSampleGradTileLaunch &a, int n_cpl, int n_cu, hipStream_t stream)
{
    if (a.H < 1 || a.W < 1 || a.H > NF_GRAD_TILE || a.W > NF_GRAD_TILE || a.H > a.img_H || a.W > a.img_W || a.tile_ny < 1 || a.tile_nx < 1 ||
        a.tile_halo < 0 || !a.g_in || a.n_cpl > n_cpl)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nf_grad_lds_floats(a.H, a.W, prog.width, n_cpl);
    if (lds > 160 * 1024 || a.gate_words != nf_grad_gate_words(n_cpl, prog.width)) return hipErrorInvalidValue;
    switch (prog.width) {
    case 4: return dispatch_sgrad_tiled<4>(prog, a, n_cu, lds, stream);
    case 8: return dispatch_sgrad_tiled<8>(prog, a, n_cu, lds, stream);
    case 16: return dispatch_sgrad_tiled<16>(prog, a, n_cu, lds, stream);
    default: return hipErrorInvalidValue;
    }
}
