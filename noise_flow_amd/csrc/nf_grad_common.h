// What the gradient kernels share: nf_grad_kernel (nf_grad.hip), nf_grad_wide_kernel (nf_grad_wide.hip), nf_grad_gemm_kernel
// (nf_grad_gemm.hip), nf_sample_grad_kernel (nf_sample_grad.hip) and nf_sample_grad_wide_kernel (nf_sample_grad_wide.hip).  Two layers:
//   (a) GradFrame, for all of them: one launch patch's view of its tensors — conditioning access, the float4 load with a fill value
//       (x, y, g_in, eps and gx_in all go through it), the 4x4 product and the pointwise layers in the NLL direction (MIX, SDN_DIV,
//       SCALE, SCALE_COND);
//   (b) GradCoupling, for nf_grad_kernel and nf_sample_grad_kernel: the gate record and the coupling CNN with scalar (SGPR) weights,
//       forward (gates recorded) and recomputed (gates replayed), by coupling index in either sweep order.
// How a pixel slot k maps to a pixel differs per kernel (precomputed arrays, or recomputed from the tile's origin): GradFrame takes a
// PIX record with act(k) and gidx(k) — GradSlotPix over a kernel's arrays, GradPix over its callables.
//
// The rule for what lives here is DESIGN 4 ("The rule"): a helper is adopted only where every kernel's instruction stream stays the
// one of the code it replaces (tools/asm_compare.py --exact, profiles/grad_common_asm.txt).  That decides the FORM and the EXTENT:
//   - what was a `[&]` lambda of a kernel is a member function WITHOUT __forceinline__ of a record of REFERENCES to the kernel's
//     variables, which is what a closure is: optimised on its own first and inlined afterwards, as the lambda was.  Forcing these
//     inline, letting a record own the slot arrays, or passing a coupling's block address or gate-set index in place of (off, cidx)
//     each moved instructions in 15 to 23 of the 23 instantiations of nf_grad_kernel.  Do not "tidy" one form into another.
//   - what stands INLINE in the kernels' bodies stays there: slot set-up and LDS carve-up, tile placement, the backward forms of the
//     pointwise layers, the transposed coupling pass, the patch reduction with the nll_b epilogue, the stores.  Each was tried as a
//     __forceinline__ helper and moved instructions (DESIGN 4.10 has the counts); the kernels say so where the code stands.
#pragma once
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nf_device.h"
#include "nf_dev_util.h"

namespace {

// ---- (a) the frame ----------------------------------------------------------------------------------------------------------

// slot k -> pixel: act(k) the slot holds a pixel, gidx(k) its index in the patch's / image's tensors.  For the kernels that hold the
// index in an array ...
template <int PX>
struct GradSlotPix {
    const bool (&act_)[PX];
    const int (&gidx_)[PX];
    __device__ __forceinline__ bool act(int k) const { return act_[k]; }
    __device__ __forceinline__ int gidx(int k) const { return gidx_[k]; }
};
// ... and for those that recompute it (gidx_: the kernel's callable)
template <int PX, typename GIDX>
struct GradPix {
    const bool (&act_)[PX];
    const GIDX &gidx_;
    __device__ __forceinline__ bool act(int k) const { return act_[k]; }
    __device__ __forceinline__ int gidx(int k) const { return gidx_(k); }
};

// z <- z M, M row-major [c][k] at P
template <int PX>
__device__ __forceinline__ void grad_mat4(const cfloat_p P, float (&z)[PX][4])
{
    float m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = P[i];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = z[k][0] * m[j];
            s = fmaf(z[k][1], m[4 + j], s);
            s = fmaf(z[k][2], m[8 + j], s);
            s = fmaf(z[k][3], m[12 + j], s);
            o[j] = s;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) z[k][j] = o[j];
    }
}

template <int PX>
__device__ __forceinline__ void grad_scale(float s, float (&z)[PX][4])
{
#pragma unroll
    for (int k = 0; k < PX; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[k][c] *= s;
}

// One launch patch's view of its tensors (the kernels' former per-patch lambdas; see the note on forms above): conditioning access,
// the float4 loads with a fill value, the pointwise ops in the NLL direction.  Refers to the kernel's own variables:
//   in4  the sweep's input (nf_nll_grad: x, TILED: z_in; nf_sample_vjp has none), y4 the clean image (neither is dereferenced by a
//   program that does not need it), both already at the patch; patch_off: the float4 offset load4 adds to a tensor's base.
template <int PX, typename ARGS, typename PIX>
struct GradFrame {
    const NfProgram &prog;
    const ARGS &a;
    const PIX &pix;
    const nf_crow_p &crow;
    const size_t &patch_off;
    const float4 *const &in4;
    const float4 *const &y4;

    __device__ float cond_a(int slot) const { return a.cond_rows ? crow->a[slot & 3] : a.cond_a[slot & 3]; }
    __device__ float cond_b(int slot) const { return a.cond_rows ? crow->b[slot & 3] : a.cond_b[slot & 3]; }

    // v = the patch's pixels of s4, `fill` in the slots without one
    __device__ __forceinline__ void fill4(const float4 *s4, float fill, float (&v)[PX][4]) const
    {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            float4 q = make_float4(fill, fill, fill, fill);
            if (pix.act(k)) q = s4[pix.gidx(k)];
            v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
        }
    }
    __device__ void load4(const float *src, float fill, float (&v)[PX][4]) const { fill4(reinterpret_cast<const float4 *>(src) + patch_off, fill, v); }
    __device__ void load_x(float (&z)[PX][4]) const { fill4(in4, 0.f, z); }
    __device__ void load_y(float (&yy)[PX][4]) const { fill4(y4, 1.f, yy); }
    __device__ void mat4(const cfloat_p P, float (&z)[PX][4]) const { grad_mat4(P, z); }

    // MIX, SDN_DIV, SCALE, SCALE_COND as nf_flow_kernel's scalar path applies them; ld: this thread's share of the log-det
    __device__ void pointwise_fwd(int op, float (&z)[PX][4], float &ld) const
    {
        const int type = prog.ops[op].type;
        const int off = prog.ops[op].off;
        if (type == NF_OP_MIX) {
            grad_mat4((cfloat_p)(a.params + off), z);
        } else if (type == NF_OP_SDN_DIV) {
            const float ck1 = cond_a(off), cb2 = cond_b(off);
            float yy[PX][4];
            load_y(yy);
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                float rp = 1.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float r = __builtin_amdgcn_rsqf(fmaf(yy[k][c], ck1, cb2));
                    z[k][c] *= r;
                    rp = c == 0 ? r : rp * r;
                }
                if (pix.act(k)) ld = fmaf(0.6931471805599453f, __builtin_amdgcn_logf(rp), ld);   // -sum_c log scale_c
            }
        } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
            grad_scale(type == NF_OP_SCALE ? ((cfloat_p)(a.params + off))[0] : cond_a(off), z);
        }
    }
};

// ---- (b) the scalar coupling pass ---------------------------------------------------------------------------------------------

// The gate record and the coupling CNN over a workgroup's pixel slots (THREADS x PX, slot k of thread t = pixel t + THREADS k; nf_device.h,
// "gate record").  Refers to the kernel's variables: t0 the z0 tile, th the relu(h2) tile, lidx / bmask a slot's index in the tiles
// and into the border table E.  LAST_FIRST: the kernel's forward sweep reaches the couplings last to first (nf_sample_vjp), so
// coupling cidx (NLL order) owns the gate sets 2 (a.n_cpl - 1 - cidx) + layer instead of 2 cidx + layer: either way the sets of a
// word are written in rising order and the one with shift 0 clears it (gate_put).
template <int WIDTH, int THREADS, int PX, typename ARGS, bool LAST_FIRST>
struct GradCoupling {
    static_assert(WIDTH == 4 || WIDTH == 8 || WIDTH == 16 || WIDTH == 32, "gate sets of WIDTH bits must tile a 32-bit word");
    static constexpr int NPIX = THREADS * PX;
    static constexpr int SPW = 32 / WIDTH;   // gate sets per word
    const ARGS &a;
    const bool (&act)[PX];
    float2 *const &t0;
    const int (&lidx)[PX];
    const int &Wp;
    uint32_t *const &gates;
    const int &t;
    float *const &th;
    const int (&bmask)[PX];

    // The first gate set of coupling cidx.  LAST_FIRST forms it once per call (`once`), the other order at every use: the kernels'
    // own forms, and each moved instructions in the other kernel when written the other way.
    __device__ __forceinline__ int gate_set_once(int cidx) const
    {
        if constexpr (LAST_FIRST) return 2 * (a.n_cpl - 1 - cidx);
        else return 0;
    }
    __device__ __forceinline__ int gate_set(int cidx, int once) const
    {
        if constexpr (LAST_FIRST) return once;
        else return 2 * cidx;
    }

    // gate set s of pixel slot k
    __device__ void gate_put(int s, int k, uint32_t bits) const
    {
        uint32_t *const p = gates + (size_t)(s / SPW) * NPIX + t + THREADS * k;
        const int sh = (s % SPW) * WIDTH;
        *p = sh == 0 ? bits : (*p | (bits << sh));
    }
    __device__ uint32_t gate_get(int s, int k) const { return gates[(size_t)(s / SPW) * NPIX + t + THREADS * k] >> ((s % SPW) * WIDTH); }

    // The coupling CNN on z0 = z[.][0:2]: o = (shift, raw log-scale) of coupling cidx, its block at a.params + off.
    // RECORD: the forward sweep — ReLU by sign, gates written to the record; otherwise the backward sweep's recomputation — ReLU by the
    // recorded gates.  Barriers: the z0 tile is free on entry (its readers passed the barrier in here), and the barrier behind its
    // publication also separates the previous readers of the h2 tile from this call's writes to it.
    template <bool RECORD>
    __device__ void cnn(int off, int cidx, const float (&z)[PX][4], float (&o)[PX][4]) const
    {
        const int once = gate_set_once(cidx);
        const cfloat_p P = (cfloat_p)(a.params + off);
#pragma unroll
        for (int k = 0; k < PX; ++k)
            if (act[k]) t0[lidx[k]] = make_float2(z[k][0], z[k][1]);
        __syncthreads();
        {
            const cfloat_p W1 = P + nf_cpl_off_W1(WIDTH);
            const cfloat_p B1 = P + nf_cpl_off_B1(WIDTH);
            const cfloat_p W2 = P + nf_cpl_off_W2(WIDTH);
            const cfloat_p B2 = P + nf_cpl_off_B2(WIDTH);
            float h1[PX][WIDTH];
#pragma unroll
            for (int k = 0; k < PX; ++k)
#pragma unroll
                for (int j = 0; j < WIDTH; ++j) h1[k][j] = B1[j];
#pragma unroll 1
            for (int di = 0; di < 3; ++di) {
                const cfloat_p W1r = W1 + di * (3 * 2 * WIDTH);
                const int roff = (di - 1) * Wp - 1;
#pragma unroll
                for (int dj = 0; dj < 3; ++dj) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const float2 v = t0[lidx[k] + roff + dj];
#pragma unroll
                        for (int j = 0; j < WIDTH; ++j) {
                            h1[k][j] = fmaf(v.x, W1r[(dj * 2 + 0) * WIDTH + j], h1[k][j]);
                            h1[k][j] = fmaf(v.y, W1r[(dj * 2 + 1) * WIDTH + j], h1[k][j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                uint32_t g1 = 0u, g2 = 0u;
                if constexpr (RECORD) {
#pragma unroll
                    for (int i = 0; i < WIDTH; ++i) g1 |= (__float_as_int(h1[k][i]) > 0 ? 1u : 0u) << i;
                    gate_put(gate_set(cidx, once), k, g1);
                } else {
                    g1 = gate_get(gate_set(cidx, once), k);
                    g2 = gate_get(gate_set(cidx, once) + 1, k);
                }
                float h2[WIDTH];
#pragma unroll
                for (int j = 0; j < WIDTH; ++j) h2[j] = B2[j];
#pragma unroll
                for (int i = 0; i < WIDTH; ++i) {
                    const float hi = RECORD ? nf_relu(h1[k][i]) : ((g1 >> i) & 1u) ? h1[k][i] : 0.0f;
#pragma unroll
                    for (int j = 0; j < WIDTH; ++j) h2[j] = fmaf(hi, W2[i * WIDTH + j], h2[j]);
                }
                if constexpr (RECORD) {
#pragma unroll
                    for (int i = 0; i < WIDTH; ++i) g2 |= (__float_as_int(h2[i]) > 0 ? 1u : 0u) << i;
                    gate_put(gate_set(cidx, once) + 1, k, g2);
                }
                if (act[k]) {
                    float4 *const dst = reinterpret_cast<float4 *>(th + (size_t)lidx[k] * WIDTH);
#pragma unroll
                    for (int q = 0; q < WIDTH / 4; ++q) {
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            v[e] = RECORD ? nf_relu(h2[4 * q + e]) : ((g2 >> (4 * q + e)) & 1u) ? h2[4 * q + e] : 0.0f;
                        dst[q] = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
        }
        __syncthreads();
        {
            const cfloat_p W3 = P + nf_cpl_off_W3(WIDTH);
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const float4 e = *reinterpret_cast<const float4 *>(a.params + off + nf_cpl_off_E(WIDTH) + 4 * bmask[k]);
                o[k][0] = e.x; o[k][1] = e.y; o[k][2] = e.z; o[k][3] = e.w;
            }
#pragma unroll 1
            for (int di = 0; di < 3; ++di) {
                const cfloat_p W3r = W3 + di * (3 * WIDTH * 4);
                const int roff = (di - 1) * Wp - 1;
#pragma unroll
                for (int dj = 0; dj < 3; ++dj) {
#pragma unroll
                    for (int q = 0; q < WIDTH / 4; ++q) {
#pragma unroll
                        for (int k = 0; k < PX; ++k) {
                            const float4 hv = *reinterpret_cast<const float4 *>(th + (size_t)(lidx[k] + roff + dj) * WIDTH + 4 * q);
                            const float hh[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int j = 0; j < 4; ++j) o[k][j] = fmaf(hh[i], W3r[(dj * WIDTH + 4 * q + i) * 4 + j], o[k][j]);
                        }
                    }
                }
            }
        }
    }

};

}  // namespace
