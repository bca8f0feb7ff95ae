// What the four GEMM kernels (nf_gemm.hip, nf_gemm16.hip: variants A and B each) share beyond nf_flow_common.h (the tile geometry, the
// input draw / load, the per-pixel layers, the affine half of a coupling behind its CNN, the epilogue, the batch sums):
//  * All four: the pixel record and the launch (one persistent workgroup per CU, pixels per thread by patch size, the per-patch-
//    conditioning instantiation, the padded width).
//  * nf_gemmb_kernel and nf_gemm16_kernel also: the frame (gemm_frame: persistent patch loop, op interpreter, epilogue, sums) and
//    the pieces of a coupling on either side of its CNN (publication of the pass-through half, bias fill of an accumulator tile,
//    P-record store, 9-tap gather).  Such a kernel is its LDS carve-up, its lane constants and the CNN it hands to gemm_frame.
//  * nf_gemm_kernel and nf_gemm16b_kernel keep their own frame, gather and stored pixel table (GemmPixTable says why).
// The CNNs themselves (three GEMMs per coupling in two operand precisions and two work splits) stay in their kernels.
//
// Pixel ownership: thread t owns pixels p = t + GT m, m < OWN (GemmPix / GemmPixTable).
//
// Replaces (reference): layers.py:251-375 (AffineCoupling, the part around the CNN).
#pragma once
#include <atomic>
#include <type_traits>
#include "nf_flow_common.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int GT = 512;          // threads per workgroup
constexpr int GW = GT / 64;      // wavefronts

__device__ __forceinline__ float4 ldg4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// The pixels a thread owns: p = t + GT m, m < OWN, at (pr(m), pc(m)) of the patch, act(m) = inside it.  Nothing is kept per pixel:
// row and column are recomputed where they are used (a division per use; the gather asks only for the few pixels that pass its
// range test).  A table would live across every CNN, where each kernel of the family is at its 256-VGPR budget.
template <int OWN>
struct GemmPix {
    int HW, W;
    __device__ __forceinline__ int p(int m) const { return (int)threadIdx.x + GT * m; }
    __device__ __forceinline__ bool act(int m) const { return p(m) < HW; }
    __device__ __forceinline__ int pr(int m) const { return act(m) ? p(m) / W : 0; }
    __device__ __forceinline__ int pc(int m) const { return act(m) ? p(m) - pr(m) * W : 0; }
};

// nf_gemm_kernel and nf_gemm16b_kernel are NOT on gemm_frame: on it (with any form of the pixel record) they lose 1 - 9 % at 8 pixels
// per thread (profiles/r10_gemm_frame_ab.txt) — the register allocation around their CNN tips over — so they keep their own frame,
// gather and pixel table pr[m] / pc[m] / act[m], and hand that table to the shared per-pixel helpers through this view.
template <int OWN>
struct GemmPixTable {
    const int (&r)[OWN], (&c)[OWN];
    const bool (&a)[OWN];
    __device__ __forceinline__ bool act(int m) const { return a[m]; }
    __device__ __forceinline__ int pr(int m) const { return r[m]; }
    __device__ __forceinline__ int pc(int m) const { return c[m]; }
};

// ---- the pieces of a coupling around its CNN -------------------------------------------------------------------------------------
// publish the pass-through half as a CNN input: the two fp32 planes z0s [2][PL] of rows Wp, tile coordinates = pixel + zb ...
template <int OWN>
__device__ __forceinline__ void gemm_publish(float *z0s, int PL, int Wp, int zb, const GemmPix<OWN> &pix, const float (&z)[OWN][4])
{
#pragma unroll
    for (int m = 0; m < OWN; ++m)
        if (pix.act(m)) {
            z0s[(pix.pr(m) + zb) * Wp + pix.pc(m) + zb] = z[m][0];
            z0s[PL + (pix.pr(m) + zb) * Wp + pix.pc(m) + zb] = z[m][1];
        }
}
// ... or rounded to half, one half2 per pixel of the bordered tile z0h (the fp16 CNNs)
template <int OWN>
__device__ __forceinline__ void gemm_publish_half(uint32_t *z0h, int Wp, const GemmPix<OWN> &pix, const float (&z)[OWN][4])
{
#pragma unroll
    for (int m = 0; m < OWN; ++m)
        if (pix.act(m)) {
            const v2h zh = {(_Float16)z[m][0], (_Float16)z[m][1]};
            z0h[(pix.pr(m) + 1) * Wp + pix.pc(m) + 1] = __builtin_bit_cast(uint32_t, zh);
        }
}

// an accumulator tile starts as its bias: b = the 16 values of this lane half (D register v = channel c(v, g))
__device__ __forceinline__ v16f gemm_acc_bias(const float *b)
{
    v16f d;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 bb = ldg4(b + 4 * q);
        d[4 * q + 0] = bb.x; d[4 * q + 1] = bb.y; d[4 * q + 2] = bb.z; d[4 * q + 3] = bb.w;
    }
    return d;
}

// One pixel's P record (NF7_P_STRIDE floats at dst): [tap 0..7][j] (register group a of lane half g holds tap 2 a + g), then tap 8 of
// lane half 0 / 1 — the 4x4 tile sums over its own half of the channels only.
__device__ __forceinline__ void gemm_store_p(float *dst, int g, const v16f &pa, const v4f &p8)
{
#pragma unroll
    for (int aa = 0; aa < 4; ++aa)
        *reinterpret_cast<float4 *>(dst + (2 * aa + g) * 4) = make_float4(pa[4 * aa + 0], pa[4 * aa + 1], pa[4 * aa + 2], pa[4 * aa + 3]);
    *reinterpret_cast<float4 *>(dst + 32 + 4 * g) = make_float4(p8[0], p8[1], p8[2], p8[3]);
}

// The 9-tap gather: the taps of the pixels [p0, p0 + np) whose P records are in LDS that fall on the output pixels this thread
// owns, o[r][c] += sum_taps P[r+di-1][c+dj-1][tap].  Pixel p0 + src has KP partial records (one per wavefront along the channel
// axis) at pp + (k kstride + rec(src)) NF7_P_STRIDE, k < KP; rec(src) < 0: not staged now.  'SAME' padding is the bounds checks.
struct GemmRecIdentity {
    __device__ __forceinline__ int operator()(int src) const { return src; }
};
template <int OWN, int KP, typename REC = GemmRecIdentity>
__device__ __forceinline__ void gemm_gather(const float *pp, int kstride, int p0, int np, int H, int W, const GemmPix<OWN> &pix, float (&o)[OWN][4],
                                            REC rec_of = REC())
{
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const int q = pix.p(m);
        if (!pix.act(m) || q + W + 1 < p0 || q >= p0 + np + W + 1) continue;
#pragma unroll
        for (int di = 0; di < 3; ++di) {
            const int rr = pix.pr(m) + di - 1;
            if (rr < 0 || rr >= H) continue;
#pragma unroll
            for (int dj = 0; dj < 3; ++dj) {
                const int cc = pix.pc(m) + dj - 1;
                const int src = rr * W + cc - p0;
                if (cc < 0 || cc >= W || src < 0 || src >= np) continue;
                const int rec = rec_of(src);
                if (rec < 0) continue;
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const float *rp = pp + ((size_t)(k * kstride + rec)) * NF7_P_STRIDE;
                    float4 v = *reinterpret_cast<const float4 *>(rp + (di * 3 + dj) * 4);
                    if (di * 3 + dj == 8) {   // tap 8: the two lane halves' partial sums
                        const float4 u = *reinterpret_cast<const float4 *>(rp + 36);
                        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
                    }
                    o[m][0] += v.x; o[m][1] += v.y; o[m][2] += v.z; o[m][3] += v.w;
                }
            }
        }
    }
}

// ---- the frame: persistent loop over the workgroup's patches, the op interpreter, epilogue, batch sums ---------------------------
//   red        [3][GW] floats of LDS
//   coupling   the kernel's CNN, force-inlined: coupling(type, op offset, P = the op's parameters, T, pix, z, o, ld2) publishes the
//              pass-through half, evaluates the CNN onto o (zero on entry) and ends in flow_finish_coupling
// Every thread of the workgroup calls this, after the kernel has zeroed its pass-through tile (and passed a barrier).
template <int OWN, bool PHILOX, bool PC, typename F>
__device__ __forceinline__ void gemm_frame(const NfProgram &prog, const NfLaunch &a, float *red, F &&coupling)
{
    const int H = a.H, W = a.W, HW = H * W;
    const GemmPix<OWN> pix = {HW, W};
    const int n_ops = prog.n_ops;
    double acc_nll = 0.0, acc_sd = 0.0;   // thread 0 only

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const FlowTile T = flow_tile<PC>(a, b, H, W);
        float z[OWN][4];
        flow_input<OWN, PHILOX>(a, T, pix, z);

        float ld = 0.0f, ld2 = 0.0f;   // natural-log / log2 parts of this thread's log-det share

        for (int op = 0; op < n_ops; ++op) {
            const int type = prog.ops[op].type;
            const cfloat_p P = (cfloat_p)(a.params + prog.ops[op].off);   // wave-uniform, scalar loads

            if (type == NF_OP_MIX) {
                flow_mix<OWN>(P, z);
            } else if (type == NF_OP_COUPLING_FWD || type == NF_OP_COUPLING_REV) {
                // the raw outputs of l_last per owned pixel; zeroed element by element: `= {}` makes the array ONE 4 OWN-wide value
                // that is copied as a whole wherever the gather's branches meet (+ 30 % vector instructions at OWN = 8)
                float o[OWN][4];
#pragma unroll
                for (int m = 0; m < OWN; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[m][j] = 0.0f;
                coupling(type, prog.ops[op].off, P, T, pix, z, o, ld2);
            } else if (type == NF_OP_SDN_DIV || type == NF_OP_SDN_MUL) {
                flow_sdn<OWN, PC>(type, prog.ops[op].off, a, T, pix, z, ld);
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                flow_scale<OWN>(type == NF_OP_SCALE ? P[0] : nf_cond_a<PC>(a, T.crow, prog.ops[op].off), z);
            }
        }

        flow_epilogue<OWN, PC, GW>(a, T, b, HW, pix, z, ld, ld2, red, acc_nll, acc_sd);
    }
    flow_flush_sums(a, acc_nll, acc_sd);
}

// ---- launching (host) ------------------------------------------------------------------------------------------------------------
// What nf_gemm.hip and nf_gemm16.hip share around their kernels.  A kernel FAMILY is a struct with
//   template <int OWN, bool PC> static auto kernel()      the __global__ function of that instantiation.

// One persistent workgroup of GT threads per CU (the band / slab images take most of a CU's LDS); per-patch conditioning
// (a.cond_rows) is the PC instantiation; dynamic LDS beyond 64 KiB is opted into once per device and kernel instantiation
// (`lds_set`: the largest size enabled so far; racy but idempotent).
template <typename FAM, int OWN, bool PC = false>
inline hipError_t gemm_launch_own(size_t lds, const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream)
{
    if constexpr (!PC) {
        if (a.cond_rows) return gemm_launch_own<FAM, OWN, true>(lds, prog, a, n_cu, device, stream);
    }
    static std::atomic<size_t> lds_set[16];
    const auto kern = FAM::template kernel<OWN, PC>();
    if (lds > FLOW_LDS_MAX) return hipErrorInvalidValue;
    std::atomic<size_t> &cur = lds_set[device & 15];
    if (lds > cur.load(std::memory_order_relaxed) || device > 15) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        cur.store(lds, std::memory_order_relaxed);
    }
    int64_t groups = n_cu;
    if (a.B < groups) groups = a.B;
    if (groups < 1) groups = 1;
    hipLaunchKernelGGL(kern, dim3((unsigned)groups), dim3(GT), lds, stream, prog, a);
    return hipGetLastError();
}

// ... with OWN = pixels per thread by patch size (2, 4 or 8: up to 64 x 64)
template <typename FAM>
inline hipError_t gemm_launch(size_t lds, const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream)
{
    const int hw = a.H * a.W;
    if (hw <= 2 * GT) return gemm_launch_own<FAM, 2>(lds, prog, a, n_cu, device, stream);
    if (hw <= 4 * GT) return gemm_launch_own<FAM, 4>(lds, prog, a, n_cu, device, stream);
    return gemm_launch_own<FAM, 8>(lds, prog, a, n_cu, device, stream);
}

// f(std::integral_constant<int, WP>, std::bool_constant<PHILOX>) for the padded width wp = 64 / 128 / 256 / 512 <= WMAX of a program
// and the input flag of a launch
template <int WMAX, typename F>
inline hipError_t gemm_by_width(int wp, const NfLaunch &a, F &&f)
{
    const auto w = [&](auto wpc) { return (a.flags & NF_K_PHILOX_IN) ? f(wpc, std::true_type{}) : f(wpc, std::false_type{}); };
    switch (wp) {
    case 64: return w(std::integral_constant<int, 64>{});
    case 128: return w(std::integral_constant<int, 128>{});
    case 256:
        if constexpr (WMAX >= 256) return w(std::integral_constant<int, 256>{});
        break;
    case 512:
        if constexpr (WMAX >= 512) return w(std::integral_constant<int, 512>{});
        break;
    }
    return hipErrorInvalidValue;
}

}  // namespace
