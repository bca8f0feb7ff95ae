// What the four GEMM kernels (nf_gemm.hip, nf_gemm16.hip: variants A and B each) share: everything AROUND the coupling CNN.
//  * All four: where a patch (or, NF_K_TILED, a tile of an image) sits, the input draw / load, the per-pixel layers (Conv2d1x1, the
//    sdn and gain families), the affine half of a coupling behind its CNN, the epilogue (prior, log-det, batch sums) — generic over
//    the pixel record — and the launch (one persistent workgroup per CU, pixels per thread by patch size, the per-patch-conditioning
//    instantiation, the padded width).
//  * nf_gemmb_kernel and nf_gemm16_kernel also: the frame (gemm_frame: persistent patch loop, op interpreter, epilogue, sums) and
//    the pieces of a coupling on either side of its CNN (publication of the pass-through half, bias fill of an accumulator tile,
//    P-record store, 9-tap gather).  Such a kernel is its LDS carve-up, its lane constants and the CNN it hands to gemm_frame.
//  * nf_gemm_kernel and nf_gemm16b_kernel keep their own frame, gather and stored pixel table (GemmPixTable says why).
// The CNNs themselves (three GEMMs per coupling in two operand precisions and two work splits) stay in their kernels.
//
// Pixel ownership: thread t owns pixels p = t + GT m, m < OWN (GemmPix / GemmPixTable).
//
// Replaces (reference, /root/reference): layers.py:108-124 (Conv2d1x1), :251-375 (AffineCoupling, the part around the CNN),
// cond_utils.py:205-239 (sdn), noise_flow_model.py:394-428, :477-478, :537-539 (objective, sd_z, prior).
#pragma once
#include <atomic>
#include <type_traits>

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

// Where this "patch" sits: on its own ([B,H,W,4] tensors), or — NF_K_TILED (nf_device.h, "overlapping tiles") — as tile
// b % tiles of image b / tiles: pixel (r, c) of the tile is pixel (oy + r, ox + c) of an IH x IW image, border masks follow the
// image border, and results are reported for the core window [cy0, cy1) x [cx0, cx1) only.
struct GemmTile {
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
__device__ __forceinline__ GemmTile gemm_tile(const NfLaunch &a, int64_t b, int H, int W)
{
    GemmTile T;
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
__device__ __forceinline__ void gemm_input(const NfLaunch &a, const GemmTile &T, const PIX &pix, float (&z)[OWN][4])
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
__device__ __forceinline__ void gemm_mix(cfloat_p P, float (&z)[OWN][4])
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
__device__ __forceinline__ void gemm_sdn(int type, int slot, const NfLaunch &a, const GemmTile &T, const PIX &pix, float (&z)[OWN][4],
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
__device__ __forceinline__ void gemm_scale(float s, float (&z)[OWN][4])
{
#pragma unroll
    for (int m = 0; m < OWN; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) z[m][q] *= s;
}

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

// The affine half of a coupling behind its CNN: o = the 4 raw outputs of l_last per owned pixel (without the border-table /
// bias entry), etab = the coupling's 16 x 4 border table, scl / m2scl = scale log2(e), -2 scale log2(e).
//   HALF   fp16-CNN layouts (the raw columns are pre-scaled by 2 log2(e) there too: inside the rounded weights, nf_host.hip::to_half_w3)
template <int OWN, bool HALF, typename PIX>
__device__ __forceinline__ void gemm_finish_coupling(int type, const float *__restrict__ etab, float scl, float m2scl, const GemmTile &T,
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

// ---- epilogue (as nf_flow_kernel): outputs, per-patch nll / sd_z / log-det or, tiled, the tile's share of its image's sums ----
//   red   [3][GW] floats of LDS;  every thread of the workgroup calls this (two barriers)
template <int OWN, bool PC, typename PIX>
__device__ __forceinline__ void gemm_epilogue(const NfLaunch &a, const GemmTile &T, int64_t b, int HW, const PIX &pix, const float (&z)[OWN][4],
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
            red[GW + wv] = r1;
            red[2 * GW + wv] = r2;
        }
        __syncthreads();
        if (t == 0) {
            r0 = 0.f; r1 = 0.f; r2 = 0.f;
#pragma unroll
            for (int i = 0; i < GW; ++i) {
                r0 += red[i];
                r1 += red[GW + i];
                r2 += red[2 * GW + i];
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
__device__ __forceinline__ void gemm_flush_sums(const NfLaunch &a, double acc_nll, double acc_sd)
{
    if (a.sums && threadIdx.x == 0 && !(a.flags & NF_K_TILED)) {
        double *sp = a.sums;
        if (a.flags & NF_K_SUMS_WIDE) sp += (size_t)(blockIdx.x & (NF_SUMS_SLOTS - 1)) * NF_SUMS_STRIDE;
        atomicAdd(&sp[0], acc_nll);
        atomicAdd(&sp[1], acc_sd);
        if (blockIdx.x == 0) atomicAdd(&sp[2], (double)a.B);
    }
}

// ---- the frame: persistent loop over the workgroup's patches, the op interpreter, epilogue, batch sums ---------------------------
//   red        [3][GW] floats of LDS
//   coupling   the kernel's CNN, force-inlined: coupling(type, op offset, P = the op's parameters, T, pix, z, o, ld2) publishes the
//              pass-through half, evaluates the CNN onto o (zero on entry) and ends in gemm_finish_coupling
// Every thread of the workgroup calls this, after the kernel has zeroed its pass-through tile (and passed a barrier).
template <int OWN, bool PHILOX, bool PC, typename F>
__device__ __forceinline__ void gemm_frame(const NfProgram &prog, const NfLaunch &a, float *red, F &&coupling)
{
    const int H = a.H, W = a.W, HW = H * W;
    const GemmPix<OWN> pix = {HW, W};
    const int n_ops = prog.n_ops;
    double acc_nll = 0.0, acc_sd = 0.0;   // thread 0 only

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const GemmTile T = gemm_tile<PC>(a, b, H, W);
        float z[OWN][4];
        gemm_input<OWN, PHILOX>(a, T, pix, z);

        float ld = 0.0f, ld2 = 0.0f;   // natural-log / log2 parts of this thread's log-det share

        for (int op = 0; op < n_ops; ++op) {
            const int type = prog.ops[op].type;
            const cfloat_p P = (cfloat_p)(a.params + prog.ops[op].off);   // wave-uniform, scalar loads

            if (type == NF_OP_MIX) {
                gemm_mix<OWN>(P, z);
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
                gemm_sdn<OWN, PC>(type, prog.ops[op].off, a, T, pix, z, ld);
            } else if (type == NF_OP_SCALE || type == NF_OP_SCALE_COND) {
                gemm_scale<OWN>(type == NF_OP_SCALE ? P[0] : nf_cond_a<PC>(a, T.crow, prog.ops[op].off), z);
            }
        }

        gemm_epilogue<OWN, PC>(a, T, b, HW, pix, z, ld, ld2, red, acc_nll, acc_sd);
    }
    gemm_flush_sums(a, acc_nll, acc_sd);
}

// ---- launching (host) ------------------------------------------------------------------------------------------------------------
// What nf_gemm.hip and nf_gemm16.hip share around their kernels.  A kernel FAMILY is a struct with
//   template <int OWN, bool PC> static auto kernel()      the __global__ function of that instantiation.
constexpr size_t GEMM_LDS_MAX = 160 * 1024;   // the LDS of a CU

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
    if (lds > GEMM_LDS_MAX) return hipErrorInvalidValue;
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
