// Input gradients of the NLL at coupling width 32 on the f32 matrix cores of gfx950 (nf_nll_grad with NF_CFG_GRAD_MFMA).
//
// The contract of nf_grad_kernel (nf_grad.hip) in the geometry of nf_wide32_kernel (nf_wide.hip): one workgroup per patch of up
// to 32x32 pixels, grid-stride over patches; a TILE is one image row on the N axis of v_mfma_f32_32x32x2_f32, a wavefront owns a
// strip of TPW = 8 rows (4 / 2 on patches of up to 16 / 8 rows, so that short patches use four wavefronts too), channels sit on M,
// so the D register v of lane half g is the B operand of K step v of the next layer.  Lane half
// g owns the pixels of the rows row0 + 2m + g of its strip (m < TPW / 2): their z, g = d nll / d z and gy live in its registers.
//   forward sweep   l_1 -> ReLU -> l_2 -> ReLU -> l_last as a register chain (l_last transposed: P = W3^T relu(h2), then the
//                   shift-add of nf_wide.hip); the sign of every D register of h1 and h2 is recorded as one bit: one 32-bit word
//                   per lane, tile and coupling (nf_device.h, NFGW_*).  z, nll_b as nf_grad_kernel forms them.
//   backward sweep  g = z, then the ops in reverse; every op rebuilds its input from its output, then transforms g.  A coupling
//                   runs the forward chain again on the z0 tile with the RECORDED gates (shift, ls), publishes d(shift, raw) into a
//                   zero-bordered tile, and chains the three transposed products through registers:
//                   l_last^T (K = 36, B operands read at the nine taps of that tile) -> gate 2 -> l_2^T -> gate 1 -> l_1^T as
//                   P[pixel][tap][2] + the same shift-add, added to g0.  h1, h2 and their gradients never exist in memory.
// 'SAME' padding: the zero borders of the two tiles, the zero-filled lane shifts and the skipped rows of the shift-add.  The border
// table E is constant and has no gradient.  Everything in front of the first coupling is computed forward from the loaded x.
// Beyond 32x32 (NF_CFG_GRAD_TILED_WIDE) the TILED instantiations run the same sweeps on one tile of an image and one segment of the
// program per launch patch, as nf_grad_kernel<.., TILED> does at the narrower widths.
// Conditioning, loads and the pointwise layers in the NLL direction are nf_grad_common.h's GradFrame, as in every gradient kernel.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <type_traits>

#include "nf_device.h"
#include "nf_dev_util.h"
#include "nf_internal.h"
#include "nf_flow_common.h"   // flow_launch: the persistent-grid launcher
#include "nf_grad_common.h"   // GradFrame

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float gw_gate(uint32_t word, int bit, float x) { return ((word >> bit) & 1u) ? x : 0.0f; }

//   NW   wavefronts (strips) of the workgroup
//   TPW  tiles (= rows of a strip) per wavefront; a lane half owns OWN = TPW / 2 of them
//   TILED  NF_CFG_GRAD_TILED_WIDE (nf_device.h, "gradient tiles"), the contract of nf_grad_kernel<.., TILED>: a "patch" of the
//          launch is one H x W tile of an img_H x img_W image and `prog` one segment.  Addresses and the index into the border table
//          E follow the IMAGE (recomputed from the tile's origin where they are used: no registers held across the sweeps); the
//          zero borders of the two LDS tiles, the lane-shift masks and the skipped rows stay the TILE's — a tile is evaluated on its
//          own, the wrong terms stay inside the halo — and only the core window is stored.  nll_b is not formed here.
template <int NW, int TPW, bool TILED = false>
__global__ __launch_bounds__(64 * NW) void nf_grad_wide_kernel(const NfProgram prog, const NfGradLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int THREADS = 64 * NW;
    constexpr int OWN = TPW / 2;
    constexpr int WP = NFGW_PITCH;
    const int H = a.H, W = a.W, HW = H * W;
    const int PL = nfgw_plane(H);
    float *const z0s = smem;                       // [2][PL] channel planes of the pass-through half
    float *const dts = z0s + 2 * PL;               // [4][PL] planes of d(shift, raw)
    float *const wblk = dts + 4 * PL;              // one coupling's block (nf_device.h, NFGW_CPL_*)
    float *const exch = wblk + NFGW_CPL_SIZE;      // [NW][2][32][4] strip-boundary rows
    uint32_t *const gates = reinterpret_cast<uint32_t *>(exch + NW * 256);   // [coupling][tile][THREADS]
    float *const red = reinterpret_cast<float *>(gates + (size_t)a.gate_words * THREADS);   // [2][NW]

    const int t = threadIdx.x;
    const int w = t >> 6, lane = t & 63, n = lane & 31, g = lane >> 5;
    const int row0 = w * TPW, c = n;
    const bool col_on = c < W;
    const float ml = n > 0 ? 1.0f : 0.0f, mr = (n < 31 && c + 1 < W) ? 1.0f : 0.0f;
    const float mg0 = g == 0 ? 1.0f : 0.0f, mg1 = g == 1 ? 1.0f : 0.0f;
    const float ml0 = ml * mg0, mr1 = mr * mg1;
    bool act[OWN];
    int gidx[OWN], lidx[OWN], bmask[OWN];
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const int r = row0 + 2 * m + g;
        act[m] = r < H && col_on;
        gidx[m] = act[m] ? r * W + c : 0;
        lidx[m] = act[m] ? (r + 1) * WP + c + 1 : 0;
        bmask[m] = act[m] ? ((r == 0 ? 1 : 0) | (r == H - 1 ? 2 : 0) | (c == 0 ? 4 : 0) | (c == W - 1 ? 8 : 0)) : 0;
    }
    // zero both tiles once: borders and the columns beyond W are never written again
    for (int i = t; i < 6 * PL; i += THREADS) smem[i] = 0.0f;
    __syncthreads();

    const int n_ops = prog.n_ops;
    const int first_cpl = a.first_cpl;
    // TILED: where the tile of the current launch patch sits in its image (wave-uniform), and what follows from it per owned pixel
    [[maybe_unused]] int oy = 0, ox = 0, cy0 = 0, cy1 = 0, cx0 = 0, cx1 = 0;
    auto gidx_of = [&](int m) {
        if constexpr (TILED) return act[m] ? (oy + row0 + 2 * m + g) * a.img_W + ox + c : 0;
        else return gidx[m];
    };
    auto bmask_of = [&](int m) {
        if constexpr (TILED) {
            const int R = oy + row0 + 2 * m + g, C = ox + c;
            return act[m] ? ((R == 0 ? 1 : 0) | (R == a.img_H - 1 ? 2 : 0) | (C == 0 ? 4 : 0) | (C == a.img_W - 1 ? 8 : 0)) : 0;
        } else {
            return bmask[m];
        }
    };
    auto own_of = [&](int m) {   // TILED: the pixel is in the tile's core window
        const int R = oy + row0 + 2 * m + g, C = ox + c;
        return act[m] && R >= cy0 && R < cy1 && C >= cx0 && C < cx1;
    };

    // one coupling's block (its first `floats`) into LDS; callers put a barrier behind it
    auto stage = [&](int off, int floats) {
        const float4 *const src = reinterpret_cast<const float4 *>(a.params + off);
        float4 *const dst = reinterpret_cast<float4 *>(wblk);
        for (int i = t; i < floats / 4; i += THREADS) dst[i] = src[i];
    };

    // Horizontal part of the shift-add of tile k and its vertical hand-over (nf_wide.hip).  Register group q of lane half g' of p
    // holds the taps  q=0: (0,0)|(2,0) from the left, q=1: (0,2)|(2,2) from the right, q=2: (0,1)|(2,1) in place,
    // q=3: (1,0)|(1,2) left | right;  pc: the centre tap.
    auto shift_add = [&](const v16f &p, const v4f &pc, int k, float (&cp)[TPW][4]) {
        float rm[4];   // g'=0: row di=0 (goes one row down), g'=1: row di=2 (goes one row up)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rm[j] = fmaf(from_next(p[4 + j]), mr, fmaf(from_prev(p[j]), ml, p[8 + j]));
            cp[k][j] += fmaf(from_next(p[12 + j]), mr1, fmaf(from_prev(p[12 + j]), ml0, pc[j]));
        }
        if (k + 1 < TPW) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cp[k + 1][j] = fmaf(rm[j], mg0, cp[k + 1][j]);
        }
        if (k > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cp[k - 1][j] = fmaf(rm[j], mg1, cp[k - 1][j]);
        }
        if constexpr (NW > 1) {
            if (k == 0 && g == 1 && row0 > 0)
                *reinterpret_cast<float4 *>(exch + (w * 2 + 1) * 128 + n * 4) = make_float4(rm[0], rm[1], rm[2], rm[3]);
            if (k == TPW - 1 && g == 0 && row0 + TPW < H)
                *reinterpret_cast<float4 *>(exch + (w * 2 + 0) * 128 + n * 4) = make_float4(rm[0], rm[1], rm[2], rm[3]);
        }
    };
    // behind the barrier: strip-boundary rows in, then each lane half finishes the rows it owns
    auto finish = [&](float (&cp)[TPW][4], float (&o)[OWN][4]) {
        if constexpr (NW > 1) {
            if (row0 > 0 && row0 < H && g == 0) {   // (a strip below the image has no row: its neighbour wrote nothing)
                const float4 v = *reinterpret_cast<const float4 *>(exch + ((w - 1) * 2 + 0) * 128 + n * 4);
                cp[0][0] += v.x; cp[0][1] += v.y; cp[0][2] += v.z; cp[0][3] += v.w;
            }
            if (row0 + TPW < H && g == 1) {
                const float4 v = *reinterpret_cast<const float4 *>(exch + ((w + 1) * 2 + 1) * 128 + n * 4);
                cp[TPW - 1][0] += v.x; cp[TPW - 1][1] += v.y; cp[TPW - 1][2] += v.z; cp[TPW - 1][3] += v.w;
            }
        }
#pragma unroll
        for (int m = 0; m < OWN; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[m][j] = half_sums(cp[2 * m][j], cp[2 * m + 1][j]);
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
        // sign, gate word written; otherwise the backward sweep's recomputation on the rebuilt z0 — ReLU by the recorded word.
        // Barriers: every LDS read of the z0 tile and of the block happens between the two barriers in here (or in front of the one
        // behind the transposed products), so the next call's writes to them, which follow that barrier, race with nothing; the
        // exchange rows are read behind the second barrier and rewritten behind the next call's first.  The border table is read
        // behind the second barrier too and therefore comes from global memory, not from the (single) LDS copy of the block, which
        // the next call's stage() may already be overwriting.
        auto coupling_cnn = [&](int off, int cidx, auto record, const float (&z)[OWN][4], float (&o)[OWN][4]) {
            constexpr bool RECORD = decltype(record)::value;
#pragma unroll
            for (int m = 0; m < OWN; ++m)
                if (act[m]) {
                    z0s[lidx[m]] = z[m][0];
                    z0s[PL + lidx[m]] = z[m][1];
                }
            stage(off, RECORD ? NFGW_CPL_BWD : NFGW_CPL_SIZE);
            __syncthreads();
            const float4 *const wb4 = reinterpret_cast<const float4 *>(wblk + NFGW_CPL_FWD);
            float cp[TPW][4];
#pragma unroll
            for (int k = 0; k < TPW; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) cp[k][j] = 0.0f;
#pragma unroll
            for (int k = 0; k < TPW; ++k) {
                const int r = row0 + k;
                if (r >= H) continue;   // wave-uniform
                uint32_t *const gp = gates + ((size_t)cidx * TPW + k) * THREADS + t;
                uint32_t gw = RECORD ? 0u : *gp;
                v16f d;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 bb = wb4[NF4_IMG_B1 / 4 + g * 4 + q];
                    d[4 * q + 0] = bb.x; d[4 * q + 1] = bb.y; d[4 * q + 2] = bb.z; d[4 * q + 3] = bb.w;
                }
                const float *const zb = z0s + g * PL + r * WP + c;   // tap (di,dj) at + di*WP + dj
#pragma unroll
                for (int grp = 0; grp < 3; ++grp) {
                    const float4 aw = wb4[NF4_IMG_A1 / 4 + grp * 64 + lane];
                    const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int tap = grp * 4 + s;
                        if (tap < 9) d = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], zb[(tap / 3) * WP + tap % 3], d, 0, 0, 0);
                    }
                }
                if constexpr (RECORD) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) gw |= (__float_as_int(d[v]) > 0 ? 1u : 0u) << v;
                }
                v16f e;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 bb = wb4[NF4_IMG_B2 / 4 + g * 4 + q];
                    e[4 * q + 0] = bb.x; e[4 * q + 1] = bb.y; e[4 * q + 2] = bb.z; e[4 * q + 3] = bb.w;
                }
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    const float4 aw = wb4[NF4_IMG_A2 / 4 + grp * 64 + lane];
                    const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int v = grp * 4 + s;
                        e = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], RECORD ? nf_relu(d[v]) : gw_gate(gw, v, d[v]), e, 0, 0, 0);
                    }
                }
                if constexpr (RECORD) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) gw |= (__float_as_int(e[v]) > 0 ? 1u : 0u) << (16 + v);
                    *gp = gw;
                }
                v16f p;
                v4f pc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int v = 0; v < 16; ++v) p[v] = 0.0f;
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    const float4 aw = wb4[NF4_IMG_A3 / 4 + grp * 64 + lane];
                    const float4 ac = wb4[NF4_IMG_A3C / 4 + grp * 8 + g * 4 + (lane & 3)];
                    const float as[4] = {aw.x, aw.y, aw.z, aw.w};
                    const float cs[4] = {ac.x, ac.y, ac.z, ac.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int v = grp * 4 + s;
                        const float h = RECORD ? nf_relu(e[v]) : gw_gate(gw, 16 + v, e[v]);
                        p = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], h, p, 0, 0, 0);
                        pc = __builtin_amdgcn_mfma_f32_4x4x1f32(cs[s], h, pc, 0, 0, 0);
                    }
                }
                shift_add(p, pc, k, cp);
            }
            __syncthreads();
            finish(cp, o);
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                const float4 eb = *reinterpret_cast<const float4 *>(a.params + off + NFGW_CPL_E + 4 * bmask_of(m));
                o[m][0] += eb.x; o[m][1] += eb.y; o[m][2] += eb.z; o[m][3] += eb.w;
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
                const float sc = P[NFGW_CPL_S];
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
            if constexpr (NW > 1) {
                __syncthreads();   // the previous patch's reader is done
                if (lane == 0) {
                    red[w] = r0;
                    red[NW + w] = r2;
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
                const float sc = P[NFGW_CPL_S];
                // d nll / d (shift, raw) of the owned pixels into the zero-bordered tile (its previous readers passed the barrier
                // inside coupling_cnn)
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
                const float4 *const wt4 = reinterpret_cast<const float4 *>(wblk + NFGW_CPL_BWD);
                float cq[TPW][4];
#pragma unroll
                for (int k = 0; k < TPW; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) cq[k][j] = 0.0f;
#pragma unroll
                for (int k = 0; k < TPW; ++k) {
                    const int r = row0 + k;
                    if (r >= H) continue;   // wave-uniform
                    const uint32_t gw = gates[((size_t)cidx * TPW + k) * THREADS + t];
                    // l_last^T: d relu(h2)[pixel][c] = sum_tap sum_j d[pixel - (tap - centre)][j] W3[tap][c][j]
                    v16f dh;
#pragma unroll
                    for (int v = 0; v < 16; ++v) dh[v] = 0.0f;
                    const float *const db = dts + g * PL + (r + 2) * WP + c + 2;   // tap (di,dj), element j = 2 (s&1) + g, at - di*WP - dj
#pragma unroll
                    for (int grp = 0; grp < 5; ++grp) {
                        const float4 aw = wt4[NFGW_BWD_A3T / 4 + grp * 64 + lane];
                        const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int st = grp * 4 + s, tap = st >> 1;
                            if (st < 18)
                                dh = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], db[2 * (st & 1) * PL - (tap / 3) * WP - tap % 3], dh, 0, 0, 0);
                        }
                    }
                    // gate 2, l_2^T
                    v16f d1;
#pragma unroll
                    for (int v = 0; v < 16; ++v) d1[v] = 0.0f;
#pragma unroll
                    for (int grp = 0; grp < 4; ++grp) {
                        const float4 aw = wt4[NFGW_BWD_A2T / 4 + grp * 64 + lane];
                        const float as[4] = {aw.x, aw.y, aw.z, aw.w};
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int v = grp * 4 + s;
                            d1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], gw_gate(gw, 16 + v, dh[v]), d1, 0, 0, 0);
                        }
                    }
                    // gate 1, l_1^T as P[pixel][tap][2] and the shift-add over the flipped taps
                    v16f p;
                    v4f pc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int v = 0; v < 16; ++v) p[v] = 0.0f;
#pragma unroll
                    for (int grp = 0; grp < 4; ++grp) {
                        const float4 aw = wt4[NFGW_BWD_A1T / 4 + grp * 64 + lane];
                        const float4 ac = wt4[NFGW_BWD_A1TC / 4 + grp * 8 + g * 4 + (lane & 3)];
                        const float as[4] = {aw.x, aw.y, aw.z, aw.w};
                        const float cs[4] = {ac.x, ac.y, ac.z, ac.w};
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int v = grp * 4 + s;
                            const float h = gw_gate(gw, v, d1[v]);
                            p = __builtin_amdgcn_mfma_f32_32x32x2f32(as[s], h, p, 0, 0, 0);
                            pc = __builtin_amdgcn_mfma_f32_4x4x1f32(cs[s], h, pc, 0, 0, 0);
                        }
                    }
                    shift_add(p, pc, k, cq);
                }
                __syncthreads();
                float ga[OWN][4];
                finish(cq, ga);
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
                    if (act[m]) o4[gidx[m]] = make_float4(gz[m][0], gz[m][1], gz[m][2], gz[m][3]);
            }
            if (a.gy_out) {
                float4 *const o4 = reinterpret_cast<float4 *>(a.gy_out) + patch_off;
#pragma unroll
                for (int m = 0; m < OWN; ++m)
                    if (act[m]) o4[gidx[m]] = make_float4(gy[m][0], gy[m][1], gy[m][2], gy[m][3]);
            }
        }
    }
}

template <int NW, int TPW, bool TILED = false>
hipError_t launch_grad_wide(const NfProgram &prog, const NfGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return flow_launch<&nf_grad_wide_kernel<NW, TPW, TILED>>(64 * NW, lds, prog, a, n_cu, dev, stream);
}

// (strip height, wavefronts) by patch height — nfgw_tpw / nfgw_waves: beyond 4 rows always four wavefronts
template <bool TILED>
hipError_t dispatch_grad_wide(const NfProgram &prog, const NfGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    if (a.H > 16) return launch_grad_wide<4, 8, TILED>(prog, a, n_cu, lds, stream);
    if (a.H > 8) return launch_grad_wide<4, 4, TILED>(prog, a, n_cu, lds, stream);
    switch (nfgw_waves(a.H)) {
    case 1: return launch_grad_wide<1, 2, TILED>(prog, a, n_cu, lds, stream);
    case 2: return launch_grad_wide<2, 2, TILED>(prog, a, n_cu, lds, stream);
    default: return launch_grad_wide<4, 2, TILED>(prog, a, n_cu, lds, stream);
    }
}

}  // namespace

// programs over the wide gradient block (nf_device.h, NFGW_*), a.gate_words = nfgw_tpw(H) words per coupling; tiled: n_cpl is at most 3
// (LDS <= 81 KiB)
hipError_t nf_launch_grad_wide(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, hipStream_t stream)
{
    static_assert(NF_GRAD_TILE == 32, "a tile is a patch the whole-patch geometry holds");
    if (prog.width != 32 || a.H < 1 || a.W < 1 || a.H > 32 || a.W > 32 || a.gate_words != nfgw_tpw(a.H) * n_cpl) return hipErrorInvalidValue;
    if (tiled && (a.H > a.img_H || a.W > a.img_W || a.tile_ny < 1 || a.tile_nx < 1 || !a.z_in)) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nfgw_lds_floats(a.H, n_cpl);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    return tiled ? dispatch_grad_wide<true>(prog, a, n_cu, lds, stream) : dispatch_grad_wide<false>(prog, a, n_cu, lds, stream);
}
