// Input gradients of the NLL (nf_nll_grad): d nll_b / d x and d nll_b / d y in evaluation mode, one fused kernel.
//
// One workgroup per patch, grid-stride over patches, the NLL-order folded program in the generic layout with scalar (SGPR)
// weights, as the scalar path of nf_flow_kernel (nf_kernels.hip).  Per patch:
//   forward sweep   the arithmetic of nf_flow_kernel's scalar path: z, nll_b — and every ReLU gate recorded as one bit
//                   (nf_device.h, "gate record");
//   backward sweep  g = d nll / d z = z, then the ops in reverse.  A normalising flow is invertible, so every op first
//                   rebuilds its input from its output and then transforms g: no activation is stored, the patch stays in
//                   registers / LDS, and HBM traffic is x and y in, gx and gy out.
// The gates come from the forward sweep, not from the rebuilt values: the result is the derivative of the function the
// forward sweep evaluated.  Everything in front of the first coupling works on values computed forward from the loaded x
// (the fp32 round trip through the stack loses ~1e-4 of x, which the leading sdn layer's gy term would inherit).
// LDS: the forward kernel's two zero-bordered tiles (z0: 2 words, relu(h2): w words per tile pixel); in the backward sweep the
// relu(h2) tile is overlaid, once consumed, by d(shift, raw) (4 words of a pixel's w) and then by d h1 (w words).
// The frame (conditioning, loads, the pointwise layers in the NLL direction) and the gate record with the coupling CNN are
// nf_grad_common.h's: the frame is shared with all gradient kernels, the coupling CNN with nf_sample_grad_kernel.
//
// TILED (NF_CFG_GRAD_TILED, nf_device.h "gradient tiles"): a "patch" of the launch is one H x W tile of an img_H x img_W image and
// `prog` one SEGMENT of the program.  The tile loads the tensor in front of the segment (z_in), runs the same forward sweep over
// the segment's ops, takes g from its own z (last segment) or from the gradient the segment behind it left (g_in), runs the same
// backward sweep and stores its CORE window only (g_out; gy_out stored or added to).  Border masks follow the image border,
// conditioning rows are per image, and nll_b is not formed here (the tiled forward launches and nf_tile_combine form it).
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

template <int WIDTH, int THREADS, int PX, bool TILED = false>
__global__ __launch_bounds__(THREADS) void nf_grad_kernel(const NfProgram prog, const NfGradLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NPIX = THREADS * PX;
    constexpr int NW = THREADS / 64;
    const int H = a.H, W = a.W, HW = H * W, Wp = W + 2;
    const int tile_px = ((H + 2) * Wp + 1) & ~1;
    float2 *const t0 = reinterpret_cast<float2 *>(smem);   // z0 tile [tile_px] float2
    float *const th = smem + 2 * tile_px;                   // relu(h2) / d(shift, raw) / d h1 tile [tile_px][WIDTH]
    uint32_t *const gates = reinterpret_cast<uint32_t *>(th + (size_t)tile_px * WIDTH);   // [gate_words][NPIX]
    float *const red = reinterpret_cast<float *>(gates + (size_t)a.gate_words * NPIX);    // [2][NW]

    // (slot set-up and carve-up stand inline here and in nf_sample_grad_kernel: as a shared helper they moved instructions)
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
    const int first_cpl = a.first_cpl;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        // Where this "patch" sits: on its own, or — TILED — as tile b % tiles of image b / tiles (nf_device.h, "overlapping tiles"):
        // addresses and border masks follow the image, own[] is the tile's core window
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
        const size_t patch_off = TILED ? (size_t)img * (size_t)a.img_H * (size_t)a.img_W : (size_t)b * (size_t)HW;
        const float4 *const x4 = reinterpret_cast<const float4 *>(TILED ? a.z_in : a.x) + patch_off;
        const float4 *const y4 = reinterpret_cast<const float4 *>(a.y) + patch_off;   // (not dereferenced when a.y is null)
        const nf_crow_p crow = (nf_crow_p)(a.cond_rows) + img;
        const GradSlotPix<PX> pix = {act, gidx};
        const GradFrame<PX, NfGradLaunch, GradSlotPix<PX>> F = {prog, a, pix, crow, patch_off, x4, y4};
        const GradCoupling<WIDTH, THREADS, PX, NfGradLaunch, false> cpl = {a, act, t0, lidx, Wp, gates, t, th, bmask};

        // ---- forward sweep ----
        float z[PX][4];
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
                float o[PX][4];
                cpl.template cnn<true>(prog.ops[op].off, cidx, z, o);
                const float sc = P[nf_cpl_off_S(WIDTH)];
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const float ls0 = sc * nf_tanh(o[k][2]);
                    const float ls1 = sc * nf_tanh(o[k][3]);
                    z[k][2] = fmaf(z[k][2], nf_exp(ls0), o[k][0]);
                    z[k][3] = fmaf(z[k][3], nf_exp(ls1), o[k][1]);
                    if (act[k]) ld += ls0 + ls1;
                }
                ++cidx;
            }
        }
        // nll_b = -(log-det) + prior, as nf_flow_kernel forms it
        if (!TILED && a.nll_out) {
            float s2 = 0.f;
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (act[k]) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) s2 = fmaf(z[k][c], z[k][c], s2);
                }
            float r0 = wave_sum(ld), r2 = wave_sum(s2);
            if constexpr (NW > 1) {
                __syncthreads();   // the previous patch's reader is done
                if ((t & 63) == 0) {
                    red[t >> 6] = r0;
                    red[NW + (t >> 6)] = r2;
                }
                __syncthreads();
                if (t == 0) {
                    r0 = 0.f;
                    r2 = 0.f;
                    for (int wv = 0; wv < NW; ++wv) {
                        r0 += red[wv];
                        r2 += red[NW + wv];
                    }
                }
            }
            if (t == 0) {
                const double n = (double)HW * 4.0;
                const double logdet = (double)r0 + (a.cond_rows ? crow->ld + a.ld_const : a.ld_const);
                a.nll_out[b] = (float)(-logdet + 0.5 * n * 1.8378770664093453 + 0.5 * (double)r2);
            }
        }

        // ---- backward sweep ----
        float g[PX][4];    // d nll / d (the tensor behind the op being undone): the prior's part is z itself
        float gy[PX][4];
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                g[k][c] = z[k][c];
                gy[k][c] = 0.0f;
            }
        if constexpr (TILED) {
            if (a.g_in) {   // not the last segment: the gradient the segment behind this one stored, whole tile
                const float4 *const g4 = reinterpret_cast<const float4 *>(a.g_in) + patch_off;
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (act[k]) v = g4[gidx[k]];
                    g[k][0] = v.x; g[k][1] = v.y; g[k][2] = v.z; g[k][3] = v.w;
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
                float o[PX][4];
                cpl.template cnn<false>(off, cidx, z, o);
                const float sc = P[nf_cpl_off_S(WIDTH)];
                float d[PX][4];   // d nll / d (shift, raw)
#pragma unroll
                for (int k = 0; k < PX; ++k) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const float th_ = nf_tanh(o[k][2 + c]);
                        const float ls = sc * th_;
                        const float e = nf_exp(ls);
                        const float z1 = (z[k][2 + c] - o[k][c]) * nf_exp(-ls);   // the coupling's input
                        const float dls = fmaf(g[k][2 + c] * z1, e, -1.0f);
                        d[k][c] = g[k][2 + c];
                        d[k][2 + c] = sc * fmaf(-th_, th_, 1.0f) * dls;
                        g[k][2 + c] *= e;
                        z[k][2 + c] = z1;
                    }
                }
                // (the transposed pass stands inline here and in nf_sample_grad_kernel: as a shared helper it moved instructions)
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
                        const uint32_t g1 = cpl.gate_get(2 * cidx, k), g2 = cpl.gate_get(2 * cidx + 1, k);
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
            } else if (type == NF_OP_MIX) {
                const cfloat_p P = (cfloat_p)(a.params + off);
                float m[16], mi[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    m[i] = P[i];
                    mi[i] = P[16 + i];
                }
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    float zi[4], gi[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float s = z[k][0] * mi[j];
                        s = fmaf(z[k][1], mi[4 + j], s);
                        s = fmaf(z[k][2], mi[8 + j], s);
                        s = fmaf(z[k][3], mi[12 + j], s);
                        zi[j] = s;
                        float q = g[k][0] * m[4 * j];
                        q = fmaf(g[k][1], m[4 * j + 1], q);
                        q = fmaf(g[k][2], m[4 * j + 2], q);
                        q = fmaf(g[k][3], m[4 * j + 3], q);
                        gi[j] = q;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        z[k][j] = zi[j];
                        g[k][j] = gi[j];
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
                float yy[PX][4];
                F.load_y(yy);
#pragma unroll
                for (int k = 0; k < PX; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float v = fmaf(yy[k][c], ck1, cb2);
                        const float r = __builtin_amdgcn_rsqf(v);
                        gy[k][c] = fmaf(0.5f * ck1 * (r * r), fmaf(-g[k][c], z[k][c], 1.0f), gy[k][c]);
                        g[k][c] *= r;
                        z[k][c] *= __builtin_amdgcn_sqrtf(v);
                    }
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                const float s = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[0] : F.cond_a(off);
                const float si = type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[1] : 1.0f / s;
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
        } else {
            if (a.gx_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gx_out) + patch_off;
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) o4[gidx[k]] = make_float4(g[k][0], g[k][1], g[k][2], g[k][3]);
            }
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (act[k]) o4[gidx[k]] = make_float4(gy[k][0], gy[k][1], gy[k][2], gy[k][3]);
            }
        }
    }
}

template <int WIDTH, int THREADS, int PX, bool TILED>
hipError_t launch_grad(const NfProgram &prog, const NfGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return flow_launch<&nf_grad_kernel<WIDTH, THREADS, PX, TILED>>(THREADS, lds, prog, a, n_cu, dev, stream);
}

// TILED: tiles are at most 32x32 (nf_device.h, NF_GRAD_TILE) — the three geometries that hold them without scratch, widths 4 / 8 / 16
template <int WIDTH, bool TILED>
hipError_t dispatch_grad(const NfProgram &prog, const NfGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    const int hw = a.H * a.W;
    if constexpr (!TILED || WIDTH <= 16) {
        if (hw <= 64) return launch_grad<WIDTH, 64, 1, TILED>(prog, a, n_cu, lds, stream);
        if (hw <= 256) return launch_grad<WIDTH, 256, 1, TILED>(prog, a, n_cu, lds, stream);
        if constexpr (WIDTH >= 32) {
            if (hw <= 1024) return launch_grad<WIDTH, 1024, 1, TILED>(prog, a, n_cu, lds, stream);
        } else {
            if (hw <= 1024) return launch_grad<WIDTH, 256, 4, TILED>(prog, a, n_cu, lds, stream);
            if constexpr (WIDTH <= 8 && !TILED) {
                if (hw <= 4096) return launch_grad<WIDTH, 1024, 4, TILED>(prog, a, n_cu, lds, stream);
            }
        }
    }
    return hipErrorInvalidValue;
}

template <bool TILED>
hipError_t dispatch_grad_width(const NfProgram &prog, const NfGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    switch (prog.width) {
    case 4: return dispatch_grad<4, TILED>(prog, a, n_cu, lds, stream);
    case 8: return dispatch_grad<8, TILED>(prog, a, n_cu, lds, stream);
    case 16: return dispatch_grad<16, TILED>(prog, a, n_cu, lds, stream);
    case 32: return dispatch_grad<32, TILED>(prog, a, n_cu, lds, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t nf_launch_grad(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, hipStream_t stream)
{
    if (tiled && (a.H > NF_GRAD_TILE || a.W > NF_GRAD_TILE || a.H > a.img_H || a.W > a.img_W || a.tile_ny < 1 || a.tile_nx < 1 || !a.z_in))
        return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nf_grad_lds_floats(a.H, a.W, prog.width, n_cpl);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    // (whole-patch instantiations first: the module keeps the kernels in the order profiles/grad_common_asm.txt was compared in)
    return !tiled ? dispatch_grad_width<false>(prog, a, n_cu, lds, stream) : dispatch_grad_width<true>(prog, a, n_cu, lds, stream);
}
