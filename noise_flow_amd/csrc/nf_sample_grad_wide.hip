// Vector-Jacobian product of sampling at coupling width 32 on the f32 matrix cores of gfx950 (nf_sample_vjp with NF_CFG_SVJP_MFMA).
//
// The contract of nf_sample_grad_kernel (nf_sample_grad.hip; its header comment is the specification: sweeps, per-op rules, eps,
// output discipline) in the geometry of nf_grad_wide_kernel (nf_grad_wide.hip): one workgroup per patch of up to 32x32 pixels,
// grid-stride over patches, a wavefront owning a strip of TPW rows, lane half g the pixels of the rows row0 + 2m + g; the handle's
// NFGW_* block, the two zero-bordered tiles, block staging, exchange rows and gate record [coupling][tile][THREADS] inside
// nfgw_lds_floats(H, n_cpl).  Conditioning, loads and the 4x4 product are GradFrame's (nf_grad_common.h).  The matrix-core pieces —
// stage, shift_add, finish, the recording / replaying coupling CNN and the transposed chain — are GradWide below: the text of
// nf_grad_wide_kernel's lambdas and of its transposed pass, as members of a record of references.  They stand in BOTH files: lifted
// into a shared header, in any of three forms, they moved instructions in all ten nf_grad_wide_kernel instantiations
// (profiles/sample_vjp_wide_asm.txt), and DESIGN 4 ("The rule") keeps such a piece where it is.  A change to one of them is made in
// nf_grad_wide.hip and here.
//   forward sweep   z = eps * temp, then the NLL-order ops LAST TO FIRST, each inverted (nf_sample's arithmetic); a coupling runs the
//                   RECORDING CNN on the pass-through half, then z1 = (z1 - shift) exp(-ls).  x_out stored if asked.
//   backward sweep  g = gx_in, then the ops FIRST TO LAST: every op transforms g (and adds to gy) from its output v, then rebuilds
//                   its input u.  A coupling runs the CNN again on z0 with the RECORDED gates, publishes d(shift, raw) into the
//                   zero-bordered tile and adds the transposed chain's result to g0.  There is no log-det term.
//   end             geps = temp g, gtemp_b = sum over the active pixels of g eps: per thread, wave_sum, then the wavefronts in index
//                   order by thread 0 — no atomics, the same bits on every run.
// The gate words are whole words written by the recording pass and indexed by coupling number: the sweep order does not matter to the
// record (the set numbering of the scalar kernel's LAST_FIRST does not arise).  eps — the caller's, or nf_sample's Philox draw zeroed
// on the lanes without a pixel — is regenerated wherever it is needed and never held across the sweeps.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <type_traits>

#include "nf_device.h"
#include "nf_dev_util.h"
#include "nf_internal.h"
#include "nf_flow_common.h"        // flow_launch: the persistent-grid launcher
#include "nf_grad_common.h"        // GradFrame

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float gw_gate(uint32_t word, int bit, float x) { return ((word >> bit) & 1u) ? x : 0.0f; }

// The matrix-core pieces of nf_grad_wide_kernel (see above), for this kernel's two sweeps.
//   NW, TPW  wavefronts of the workgroup, tiles per wavefront (nf_grad_wide.hip)
//   ARGS     the launch record: params, gate record sized by a.gate_words
//   BMASK    callable m -> the index of owned pixel m into the border table E (0 where the slot holds no pixel)
// Refers to the kernel's variables: the LDS carve-up (z0s [2][PL], dts [4][PL], wblk, exch, gates), the lane's place (t, w, lane, n, g,
// row0, c), the lane-shift masks (ml, mr, mg0, mg1, ml0, mr1) and the owned pixels (act, lidx).
template <int NW, int TPW, typename ARGS, typename BMASK>
struct GradWide {
    static constexpr int THREADS = 64 * NW;
    static constexpr int OWN = TPW / 2;
    static constexpr int WP = NFGW_PITCH;
    const ARGS &a;
    const int &H;
    const int &PL;
    float *const &z0s;
    float *const &dts;
    float *const &wblk;
    float *const &exch;
    uint32_t *const &gates;
    const int &t, &w, &lane, &n, &g, &row0, &c;
    const float &ml, &mr, &mg0, &mg1, &ml0, &mr1;
    const bool (&act)[OWN];
    const int (&lidx)[OWN];
    const BMASK &bmask_of;

    // one coupling's block (its first `floats`) into LDS; callers put a barrier behind it
    __device__ void stage(int off, int floats) const
    {
        const float4 *const src = reinterpret_cast<const float4 *>(a.params + off);
        float4 *const dst = reinterpret_cast<float4 *>(wblk);
        for (int i = t; i < floats / 4; i += THREADS) dst[i] = src[i];
    }

    // Horizontal part of the shift-add of tile k and its vertical hand-over (nf_wide.hip).  Register group q of lane half g' of p
    // holds the taps  q=0: (0,0)|(2,0) from the left, q=1: (0,2)|(2,2) from the right, q=2: (0,1)|(2,1) in place,
    // q=3: (1,0)|(1,2) left | right;  pc: the centre tap.
    __device__ void shift_add(const v16f &p, const v4f &pc, int k, float (&cp)[TPW][4]) const
    {
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
    }
    // behind the barrier: strip-boundary rows in, then each lane half finishes the rows it owns
    __device__ void finish(float (&cp)[TPW][4], float (&o)[OWN][4]) const
    {
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
    }

    // The coupling CNN on z0 = z[.][0:2]: o = (shift, raw log-scale) of the owned pixels.  RECORD: the sweep that evaluates the
    // function — ReLU by sign, gate word written; otherwise the other sweep's recomputation on the rebuilt z0 — ReLU by the recorded
    // word.  Barriers: every LDS read of the z0 tile and of the block happens between the two barriers in here (or in front of the one
    // behind the transposed products), so the next call's writes to them, which follow that barrier, race with nothing; the
    // exchange rows are read behind the second barrier and rewritten behind the next call's first.  The border table is read
    // behind the second barrier too and therefore comes from global memory, not from the (single) LDS copy of the block, which
    // the next call's stage() may already be overwriting.
    template <typename REC>
    __device__ void coupling_cnn(int off, int cidx, REC record, const float (&z)[OWN][4], float (&o)[OWN][4]) const
    {
        constexpr bool RECORD = REC::value;
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
    }

    // The transposed chain of coupling cidx: ga[.][0:2] = CNN^T(d(shift, raw)) of the owned pixels, d(shift, raw) read at the nine taps
    // of the zero-bordered dts tile (published and barriered by the caller), through the RECORDED gates and the BWD images of the
    // block coupling_cnn staged whole (RECORD = false).  Ends behind its own barrier and finish().
    __device__ void transposed(int cidx, float (&ga)[OWN][4]) const
    {
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
        finish(cq, ga);
    }
};

template <int NW, int TPW>
__global__ __launch_bounds__(64 * NW) void nf_sample_grad_wide_kernel(const NfProgram prog, const NfSampleGradLaunch a)
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
    float *const red = reinterpret_cast<float *>(gates + (size_t)a.gate_words * THREADS);   // [NW] of the budgeted [2][NW]

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
    auto bmask_of = [&](int m) { return bmask[m]; };
    // zero both tiles once: borders and the columns beyond W are never written again
    for (int i = t; i < 6 * PL; i += THREADS) smem[i] = 0.0f;
    __syncthreads();

    const int n_ops = prog.n_ops;
    const int last_cpl = a.last_cpl;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const size_t patch_off = (size_t)b * (size_t)HW;
        const float4 *const y4 = reinterpret_cast<const float4 *>(a.y) + patch_off;   // (not dereferenced when a.y is null)
        const nf_crow_p crow = (nf_crow_p)(a.cond_rows) + b;
        const float4 *const no_in4 = nullptr;   // (the sweep starts from eps: GradFrame::load_x is not used)
        const GradSlotPix<OWN> pix = {act, gidx};
        const GradFrame<OWN, NfSampleGradLaunch, GradSlotPix<OWN>> F = {prog, a, pix, crow, patch_off, no_in4, y4};
        const GradWide<NW, TPW, NfSampleGradLaunch, decltype(bmask_of)> G = {a, H, PL, z0s, dts, wblk, exch, gates, t, w, lane, n, g, row0, c,
                                                                             ml, mr, mg0, mg1, ml0, mr1, act, lidx, bmask_of};

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
                G.coupling_cnn(prog.ops[op].off, cidx, std::true_type{}, z, o);
                const float sc = P[NFGW_CPL_S];
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
                G.coupling_cnn(off, cidx, std::false_type{}, z, o);
                const float sc = P[NFGW_CPL_S];
                // d L / d (shift, raw) of the owned pixels into the zero-bordered tile (its previous readers passed the barrier
                // inside coupling_cnn)
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
                float ga[OWN][4];
                G.transposed(cidx, ga);
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
            if constexpr (NW > 1) {
                __syncthreads();   // the previous patch's reader is done
                if (lane == 0) red[w] = r;
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

template <int NW, int TPW>
hipError_t launch_sgrad_wide(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, size_t lds, hipStream_t stream)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return flow_launch<&nf_sample_grad_wide_kernel<NW, TPW>>(64 * NW, lds, prog, a, n_cu, dev, stream);
}

}  // namespace

// entry point used by nf_host.hip (which has checked the supported set: sample_vjp_support); programs over the wide gradient block
// (nf_device.h, NFGW_*), a.gate_words = nfgw_tpw(H) words per coupling.  (Strip height, wavefronts) by patch height as
// nf_grad_wide.hip's dispatch_grad_wide.
hipError_t nf_launch_sample_grad_wide(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, hipStream_t stream)
{
    if (prog.width != 32 || a.H < 1 || a.W < 1 || a.H > 32 || a.W > 32 || a.n_cpl < 0 || a.gate_words != nfgw_tpw(a.H) * a.n_cpl)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * nfgw_lds_floats(a.H, a.n_cpl);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (a.H > 16) return launch_sgrad_wide<4, 8>(prog, a, n_cu, lds, stream);
    if (a.H > 8) return launch_sgrad_wide<4, 4>(prog, a, n_cu, lds, stream);
    switch (nfgw_waves(a.H)) {
    case 1: return launch_sgrad_wide<1, 2>(prog, a, n_cu, lds, stream);
    case 2: return launch_sgrad_wide<2, 2>(prog, a, n_cu, lds, stream);
    default: return launch_sgrad_wide<4, 2>(prog, a, n_cu, lds, stream);
    }
}
