// What the fused kernels share outside nf_dev_util.h:
//  * the persistent-grid launcher of every kernel that sizes its grid by occupancy (flow_launch: nf_kernels.hip, nf_wide.hip,
//    nf_wide16.hip, nf_grad.hip, nf_grad_wide.hip);
//  * where a patch or, NF_K_TILED, a tile of an image sits (FlowTile, flow_tile: nf_wide16.hip and the four GEMM kernels);
//  * everything AROUND the coupling CNN that is per pixel or per patch, generic over a PIXEL RECORD — the input draw / load, the
//    per-pixel layers (Conv2d1x1, the sdn and gain families), the affine half of a coupling behind its CNN, the epilogue (prior, sd_z,
//    log-det, tile share) and the batch sums.  The four GEMM kernels are on these (nf_gemm_common.h has their records).  nf_wide.hip
//    and nf_wide16.hip restate them inline: on the helpers their register allocation moves and they lose 5 - 12 % (width 32 fp16 at
//    32x32, width 16 at every shape: profiles/r15_wide_common_ab.txt), and nf_kernels.hip keeps its own per-pixel code.  A change to
//    one of these layers is made here and in those three files.
//
// A pixel record `pix` says which OWN pixels a thread holds in z[OWN][4]:
//   pix.act(m)            pixel m is inside the patch (and this thread's to compute)
//   pix.pr(m), pix.pc(m)  its row and column in the patch (read only where act(m), or through FlowTile::gi, which masks)
//
// Replaces (reference): layers.py:108-124 (Conv2d1x1), :251-375 (AffineCoupling, the part around the CNN),
// cond_utils.py:205-239 (sdn), noise_flow_model.py:394-428, :477-478, :537-539 (objective, sd_z, prior).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "../../include/noiseflow_hip.h"   // NF_SUMS_SLOTS / NF_SUMS_STRIDE
#include "nf_device.h"
#include "nf_dev_util.h"

namespace {

// Where this "patch" sits: on its own ([B,H,W,4] tensors), or — NF_K_TILED (nf_device.h, "overlapping tiles") — as tile
// b % tiles of image b / tiles: pixel (r, c) of the tile is pixel (oy + r, ox + c) of an IH x IW image, border masks follow the
// image border, and results are reported for the core window [cy0, cy1) x [cx0, cx1) only.
struct FlowTile {
    size_t patch_off;    // floats in front of the patch's / image's tensor
    int64_t patch_id;    // Philox key
    nf_crow_p crow;      // per-patch conditioning: this patch's (tiled: this image's) row, or null (nf_dev_util.h)
    int oy, ox, IH, IW, cy0, cy1, cx0, cx1;
    bool tiled;
    __device__ __forceinline__ int gi(bool act, int r, int c) const { return act ? (oy + r) * IW + ox + c : 0; }   // index in the tensors
    __device__ __forceinline__ bool own(bool act, int r, int c) const                                               // reported by this launch
    {
        const int R = oy + r, C = ox + c;
        return act && R >= cy0 && R < cy1 && C >= cx0 && C < cx1;
    }
    __device__ __forceinline__ int border(int r, int c) const    // index into a coupling's 16-entry border table
    {
        return (oy + r == 0 ? 1 : 0) | (oy + r == IH - 1 ? 2 : 0) | (ox + c == 0 ? 4 : 0) | (ox + c == IW - 1 ? 8 : 0);
    }
};

template <bool PC>
__device__ __forceinline__ FlowTile flow_tile(const NfLaunch &a, int64_t b, int H, int W)
{
    FlowTile T;
    T.patch_off = (size_t)b * (size_t)(H * W) * 4u;
    T.patch_id = b;
    T.oy = 0; T.ox = 0; T.IH = H; T.IW = W; T.cy0 = 0; T.cy1 = H; T.cx0 = 0; T.cx1 = W;
    T.tiled = (a.flags & NF_K_TILED) != 0;
    if (T.tiled) {
        const int nt = a.tile_ny * a.tile_nx;
        const int64_t img = b / nt;
        const int ti = (int)(b - img * nt);
        const int ty = ti / a.tile_nx, tx = ti - ty * a.tile_nx;
        T.IH = a.img_H;
        T.IW = a.img_W;
        T.oy = nf_tile_origin(ty, T.IH, H, a.tile_halo);
        T.ox = nf_tile_origin(tx, T.IW, W, a.tile_halo);
        T.cy0 = nf_tile_core0(ty, T.IH, H, a.tile_halo);
        T.cy1 = nf_tile_core1(ty, a.tile_ny, T.IH, H, a.tile_halo);
        T.cx0 = nf_tile_core0(tx, T.IW, W, a.tile_halo);
        T.cx1 = nf_tile_core1(tx, a.tile_nx, T.IW, W, a.tile_halo);
        T.patch_off = (size_t)img * (size_t)T.IH * (size_t)T.IW * 4u;
        T.patch_id = img;
    }
    T.crow = nf_cond_row_of<PC>(a, T.patch_id);
    return T;
}

// the 4 channels of each owned pixel -> registers: the in-kernel Philox / Box-Muller draw, or the input tensor
template <int OWN, bool PHILOX, typename PIX>
__device__ __forceinline__ void flow_input(const NfLaunch &a, const FlowTile &T, const PIX &pix, float (&z)[OWN][4])
{
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const int gi = T.gi(pix.act(m), pix.pr(m), pix.pc(m));
        if (PHILOX) {
            philox_normal4(a.seed, a.patch_base + T.patch_id, (uint32_t)gi, NF_STREAM_SAMP, z[m]);
#pragma unroll
            for (int q = 0; q < 4; ++q) z[m][q] *= a.in_scale;
        } else {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pix.act(m)) v = reinterpret_cast<const float4 *>(a.in + T.patch_off)[gi];
            z[m][0] = v.x * a.in_scale;
            z[m][1] = v.y * a.in_scale;
            z[m][2] = v.z * a.in_scale;
            z[m][3] = v.w * a.in_scale;
        }
    }
}

// Conv2d1x1 (and whatever was folded into it): z <- z @ M, M = P[0..15] row-major (wave-uniform scalar loads)
template <int OWN>
__device__ __forceinline__ void flow_mix(cfloat_p P, float (&z)[OWN][4])
{
    float mm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) mm[i] = P[i];
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = z[m][0] * mm[j];
            s = fmaf(z[m][1], mm[4 + j], s);
            s = fmaf(z[m][2], mm[8 + j], s);
            s = fmaf(z[m][3], mm[12 + j], s);
            o[j] = s;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) z[m][j] = o[j];
    }
}

// AffineCouplingSdnEx5 and its relatives: scale = sqrt(beta1*y/gain + beta2)  (cond_utils.py:238)
template <int OWN, bool PC, typename PIX>
__device__ __forceinline__ void flow_sdn(int type, int slot, const NfLaunch &a, const FlowTile &T, const PIX &pix, float (&z)[OWN][4],
                                         float &ld)
{
    const float4 *y4 = reinterpret_cast<const float4 *>(a.y + T.patch_off);
    const float ck1 = nf_cond_a<PC>(a, T.crow, slot), cb2 = nf_cond_b<PC>(a, T.crow, slot);
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        float4 yv = make_float4(1.f, 1.f, 1.f, 1.f);
        if (pix.act(m)) yv = y4[T.gi(pix.act(m), pix.pr(m), pix.pc(m))];
        const bool own = T.own(pix.act(m), pix.pr(m), pix.pc(m));
        const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = fmaf(yy[q], ck1, cb2);
            if (type == NF_OP_SDN_DIV) {
                z[m][q] = z[m][q] * __builtin_amdgcn_rsqf(v);
                if (own) ld = fmaf(-0.34657359027997264f, __builtin_amdgcn_logf(v), ld);
            } else {
                z[m][q] = z[m][q] * __builtin_amdgcn_sqrtf(v);
            }
        }
    }
}

template <int OWN>
__device__ __forceinline__ void flow_scale(float s, float (&z)[OWN][4])
{
#pragma unroll
    for (int m = 0; m < OWN; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) z[m][q] *= s;
}

// The affine half of a coupling behind its CNN: o = the 4 raw outputs of l_last per owned pixel (without the border-table /
// bias entry), etab = the coupling's 16 x 4 border table, scl / m2scl = scale log2(e), -2 scale log2(e).
//   HALF   fp16-CNN layouts (the raw columns are pre-scaled by 2 log2(e) there too: inside the rounded weights, nf_host.hip::to_half_w3)
template <int OWN, bool HALF, typename PIX>
__device__ __forceinline__ void flow_finish_coupling(int type, const float *__restrict__ etab, float scl, float m2scl, const FlowTile &T,
                                                     const PIX &pix, float (&o)[OWN][4], float (&z)[OWN][4], float &ld2)
{
#pragma unroll
    for (int m = 0; m < OWN; ++m) {
        const float4 eb = *reinterpret_cast<const float4 *>(etab + 4 * (pix.act(m) ? T.border(pix.pr(m), pix.pc(m)) : 0));
        o[m][0] += eb.x; o[m][1] += eb.y;
        o[m][2] += eb.z; o[m][3] += eb.w;
        // raw columns pre-scaled by 2 log2(e):  t = exp2(raw') = exp(2 raw);
        // ls*log2(e) = scl*tanh(raw) = scl - 2 scl/(t + 1); log-det accumulated in log2 units
        const float l0 = fmaf(__builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(o[m][2]) + 1.0f), m2scl, scl);
        const float l1 = fmaf(__builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(o[m][3]) + 1.0f), m2scl, scl);
        if (type == NF_OP_COUPLING_FWD) {
            z[m][2] = fmaf(z[m][2], __builtin_amdgcn_exp2f(l0), o[m][0]);
            z[m][3] = fmaf(z[m][3], __builtin_amdgcn_exp2f(l1), o[m][1]);
            if (T.own(pix.act(m), pix.pr(m), pix.pc(m))) ld2 += l0 + l1;
        } else {
            z[m][2] = (z[m][2] - o[m][0]) * __builtin_amdgcn_exp2f(-l0);
            z[m][3] = (z[m][3] - o[m][1]) * __builtin_amdgcn_exp2f(-l1);
        }
    }
}

// ---- epilogue (as nf_flow_kernel of nf_kernels.hip): outputs, per-patch nll / sd_z / log-det or, tiled, the tile's share of its image's sums ----
//   NW        wavefronts of the workgroup;  red  [3][NW] floats of LDS;  every thread of the workgroup calls this (two barriers)
template <int OWN, bool PC, int NW, typename PIX>
__device__ __forceinline__ void flow_epilogue(const NfLaunch &a, const FlowTile &T, int64_t b, int HW, const PIX &pix, const float (&z)[OWN][4],
                                              float ld, float ld2, float *red, double &acc_nll, double &acc_sd)
{
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    if (a.out) {
        float4 *out4 = reinterpret_cast<float4 *>(a.out + T.patch_off);
#pragma unroll
        for (int m = 0; m < OWN; ++m)
            if (T.own(pix.act(m), pix.pr(m), pix.pc(m))) out4[T.gi(pix.act(m), pix.pr(m), pix.pc(m))] = make_float4(z[m][0], z[m][1], z[m][2], z[m][3]);
    }
    if (a.nll_out || a.sd_out || a.ld_out || a.sums || (T.tiled && a.tile_part)) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int m = 0; m < OWN; ++m)
            if (T.own(pix.act(m), pix.pr(m), pix.pc(m))) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    s1 += z[m][q];
                    s2 = fmaf(z[m][q], z[m][q], s2);
                }
            }
        float r0 = wave_sum(fmaf(ld2, 0.6931471805599453f, ld)), r1 = wave_sum(s1), r2 = wave_sum(s2);
        if (lane == 0) {
            red[wv] = r0;
            red[NW + wv] = r1;
            red[2 * NW + wv] = r2;
        }
        __syncthreads();
        if (t == 0) {
            r0 = 0.f; r1 = 0.f; r2 = 0.f;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                r0 += red[i];
                r1 += red[NW + i];
                r2 += red[2 * NW + i];
            }
        }
        if (t == 0 && T.tiled) {
            // the tile's share of its image's sums (nf_tile_combine_kernel forms nll / sd / log-det per image)
            *reinterpret_cast<float4 *>(a.tile_part + (size_t)b * 4u) = make_float4(r0, r1, r2, 0.f);
        } else if (t == 0) {
            const double npx = (double)HW * 4.0;
            const double logdet = (double)r0 + nf_cond_ld<PC>(a, T.crow);
            double nll = -logdet;   // prior: sum -0.5*(log 2pi + z^2)   (noise_flow_model.py:537-539)
            if (a.flags & NF_K_PRIOR) nll += 0.5 * npx * 1.8378770664093453 + 0.5 * (double)r2;
            const double mean = (double)r1 / npx;
            double var = (double)r2 / npx - mean * mean;   // noise_flow_model.py:477-478
            var = var > 0.0 ? var : 0.0;
            const double sd = sqrt(var);
            if (a.nll_out) a.nll_out[b] = (float)nll;
            if (a.sd_out) a.sd_out[b] = (float)sd;
            if (a.ld_out) a.ld_out[b] = (float)logdet;
            acc_nll += (double)(float)nll;
            acc_sd += (double)(float)sd;
        }
        __syncthreads();   // scratch is reused by the next patch
    }
}

// the workgroup's share of the call's batch sums (thread 0)
__device__ __forceinline__ void flow_flush_sums(const NfLaunch &a, double acc_nll, double acc_sd)
{
    if (a.sums && threadIdx.x == 0 && !(a.flags & NF_K_TILED)) {
        double *sp = a.sums;
        if (a.flags & NF_K_SUMS_WIDE) sp += (size_t)(blockIdx.x & (NF_SUMS_SLOTS - 1)) * NF_SUMS_STRIDE;
        atomicAdd(&sp[0], acc_nll);
        atomicAdd(&sp[1], acc_sd);
        if (blockIdx.x == 0) atomicAdd(&sp[2], (double)a.B);
    }
}

// ---- launching (host) ------------------------------------------------------------------------------------------------------------
constexpr size_t FLOW_LDS_MAX = 160 * 1024;   // the LDS of a CU

// The persistent grid of a kernel whose workgroups stride over the batch: exactly the resident capacity, groups = min(B, CUs x
// resident workgroups per CU), the latter from the occupancy query for (threads, lds) clamped to 1 .. 32.  KERN is the __global__
// function (prog, a); ARGS its launch struct (NfLaunch / NfGradLaunch).  One cache entry per kernel symbol:
// (device << 40 | lds bytes << 8 | resident workgroups per CU) of the last query; racy but idempotent.  The opt-in to dynamic LDS
// beyond 64 KiB is a per-device function attribute, so the device is part of the key.
template <auto KERN, typename ARGS>
inline hipError_t flow_launch(int threads, size_t lds, const NfProgram &prog, const ARGS &a, int n_cu, int device, hipStream_t stream)
{
    if (lds > FLOW_LDS_MAX) return hipErrorInvalidValue;
    const void *fn = reinterpret_cast<const void *>(KERN);
    static std::atomic<uint64_t> cache{0};
    const uint64_t key = ((uint64_t)(device & 0xff) << 40) | ((uint64_t)lds << 8);
    const uint64_t cv = cache.load(std::memory_order_relaxed);
    int occ;
    if ((cv & ~(uint64_t)0xff) == key && (cv & 0xff) != 0) {
        occ = (int)(cv & 0xff);
    } else {
        if (lds > 64 * 1024) {   // always the CU's whole 160 KiB: concurrent callers with other patch sizes or models never lower it under a launch
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLOW_LDS_MAX);
            if (e != hipSuccess) return e;
        }
        occ = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, lds);
        if (e != hipSuccess) return e;
        if (occ < 1) occ = 1;
        if (occ > 32) occ = 32;
        cache.store(key | (uint64_t)occ, std::memory_order_relaxed);
    }
    int64_t groups = (int64_t)n_cu * occ;
    if (a.B < groups) groups = a.B;
    if (groups < 1) groups = 1;
    hipLaunchKernelGGL(KERN, dim3((unsigned)groups), dim3((unsigned)threads), lds, stream, prog, a);
    return hipGetLastError();
}

}  // namespace
