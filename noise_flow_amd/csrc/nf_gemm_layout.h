// fp16-CNN GEMM layout (NF_CFG_FP16_CNN at coupling widths 33 .. 512, nf_gemm16.hip) — kept out of nf_device.h on purpose:
// profiles/traffic.json is stamped with a content hash of the headers the HEADLINE kernel includes.
//
// Same structure as NF7_* (nf_device.h) on v_mfma_f32_32x32x16_f16 (K = 16 per instruction, fp32 accumulate): an A / B operand
// is 8 halves = 4 dwords per lane, the K slice of lane half g being elements 8g .. 8g+7.  Folded weights and the three CNN
// inputs (z0, relu(h1), relu(h2)) are rounded to half once; biases, border table, tanh / exp, log-det stay fp32 (the rounding
// points of NF3_* / NF5_* and of the oracle's cnn_dtype='fp16').  WP = the width zero-padded to 64 / 128 / 256 / 512,
// MT = WP / 32; a band = 65536 / WP pixels (h1 of the band in half precision = 128 KiB of LDS).  Offsets in dwords:
//   COUPLING  E [16][4] @0 (raw columns pre-scaled by 2 log2 e), S [4] @64, IMG8 @68:
//     A1H [MT][2][64][4]       l_1 of output tile m, 2 instructions: #0 element q of lane half g = (tap 4g + q/2, ch q&1);
//                              #1: g = 0, q < 2 = (tap 8, ch q)
//     B1  [MT][2][16]          fp32 bias by (m, g, v): b1[32 m + c(v, g)]
//     B2  [MT][2][16]
//     A2H [MT][WP/16][64][4]   l_2 of output tile m: K step ks consumes registers 8 (ks & 1) .. +7 of input tile ks / 2:
//                              element q of lane l: W2[in = 32 (ks/2) + c(8 (ks&1) + q, l>>5)][out = 32 m + (l&31)]
//     A3H [MT][2][64][4]       P = W3^T h2, taps 0 .. 7: row i = l&31 = 4 tap + j; instruction m2 of input tile mi, element q:
//                              W3[tap][in = 32 mi + c(8 m2 + q, l>>5)][j]        (NOT pre-scaled: the kernel scales in fp32)
//     A3CH[MT][4][8][2]        tap 8 on v_mfma_f32_4x4x4_16b_f16: instruction q4 of input tile mi, (g, j):
//                              W3[8][32 mi + c(4 q4 .. 4 q4 + 3, g)][j]
#pragma once
#define NF8_CPL_E 0
#define NF8_CPL_S 64
#define NF8_CPL_IMG 68
__host__ __device__ constexpr int nf8_img_A1H(int) { return 0; }
__host__ __device__ constexpr int nf8_img_B1(int wp) { return (wp / 32) * 512; }
__host__ __device__ constexpr int nf8_img_B2(int wp) { return (wp / 32) * 544; }
__host__ __device__ constexpr int nf8_img_A2H(int wp) { return (wp / 32) * 576; }
__host__ __device__ constexpr int nf8_img_A3H(int wp) { return (wp / 32) * 576 + wp * wp / 2; }
__host__ __device__ constexpr int nf8_img_A3CH(int wp) { return (wp / 32) * 576 + wp * wp / 2 + (wp / 32) * 512; }
__host__ __device__ constexpr int nf8_img_size(int wp) { return (wp / 32) * (576 + 512 + 64) + wp * wp / 2; }
__host__ __device__ constexpr int nf8_cpl_size(int wp) { return NF8_CPL_IMG + nf8_img_size(wp); }
#define NF8_BAND_HALVES 65536   // hidden activations of one band: WP channels x NB pixels, half precision (128 KiB of LDS)

// ---- variant B (pixel tiles per wavefront, weights through LDS): one contiguous SLAB per channel tile m ----------------------------
//   IMG9 @68:  A1H [MT][2][64][4] and B1 [MT][2][16] as NF8 (same offsets), then
//     SLAB [MT] x { A2H(m) [WP/16][64][4]   the l_2 rows of OUTPUT tile m, K step ks at + 64 ks (16 bytes per lane)
//                   A3H(m) [2][64][4]        the l_last columns (taps 0 .. 7) of INPUT tile m
//                   A3CH(m)[4][8][2]         tap 8
//                   B2(m)  [2][16] }         fp32 bias of l_2's output tile m
__host__ __device__ constexpr int nf9_slab_dwords(int wp) { return (wp / 16) * 256 + 512 + 64 + 32; }
__host__ __device__ constexpr int nf9_slab_A3H(int wp) { return (wp / 16) * 256; }
__host__ __device__ constexpr int nf9_slab_A3CH(int wp) { return (wp / 16) * 256 + 512; }
__host__ __device__ constexpr int nf9_slab_B2(int wp) { return (wp / 16) * 256 + 512 + 64; }
__host__ __device__ constexpr int nf9_img_SLAB(int wp) { return (wp / 32) * 544; }
__host__ __device__ constexpr int nf9_img_size(int wp) { return (wp / 32) * 544 + (wp / 32) * nf9_slab_dwords(wp); }
__host__ __device__ constexpr int nf9_cpl_size(int wp) { return NF8_CPL_IMG + nf9_img_size(wp); }

// ---- exact-fp32 variant B (nf_gemm.hip, widths <= 128): the NF7_* values, one contiguous SLAB per channel tile m ---------------------
//   IMG10 @68:  A1 [MT][3][64][4], B1 [MT][2][16] as NF7 (same offsets; NF7's B2 block stays where it is, unused), then at
//   nf10_img_SLAB:  SLAB [MT] x { A2(m) [WP/8][64][4]   l_2 rows of OUTPUT tile m, chunk kc (4 K steps) at + 256 kc floats
//                                 A3(m) [4][64][4]       l_last columns (taps 0 .. 7) of INPUT tile m
//                                 A3C(m)[4][8][4]        tap 8 (v_mfma_f32_4x4x1)
//                                 B2(m) [2][16] }
__host__ __device__ constexpr int nf10_slab_floats(int wp) { return 32 * wp + 1024 + 128 + 32; }
__host__ __device__ constexpr int nf10_slab_A3(int wp) { return 32 * wp; }
__host__ __device__ constexpr int nf10_slab_A3C(int wp) { return 32 * wp + 1024; }
__host__ __device__ constexpr int nf10_slab_B2(int wp) { return 32 * wp + 1024 + 128; }
__host__ __device__ constexpr int nf10_img_SLAB(int wp) { return (wp / 32) * 832; }
__host__ __device__ constexpr int nf10_img_size(int wp) { return (wp / 32) * 832 + (wp / 32) * nf10_slab_floats(wp); }
__host__ __device__ constexpr int nf10_cpl_size(int wp) { return 68 + nf10_img_size(wp); }

// ---- input gradients at coupling widths 33 .. 512 (nf_grad_gemm.hip, NF_CFG_GRAD_GEMM) ---------------------------------------------
// Same launch record (NfGradLaunch) and op list as the other gradient kernels; MIX and SCALE as the scalar gradient block.  Per
// coupling the block carries, in the tile / lane / register conventions of NF7_* (nf_device.h) and with nothing pre-scaled (tanh / exp
// are nf_tanh / nf_exp as in nf_grad.hip), every weight in the fetch order of v_mfma_f32_32x32x2_f32 — for the forward chain and for
// the three transposed products.  WP = the width zero-padded to 64 / 128 / 256 / 512, MT = WP / 32; a padded channel is zero in all:
//   COUPLING  E [16][4] @0 (generic values), S [4] @64 (rescaling_scale, 0, 0, 0),
//             FWD @68: the NF7 image (nf7_img_*: A1, B1, B2, A2, A3, A3C) without the 2 log2(e) factor
//             BWD @68 + nf7_img_size(WP):
//               A3T [MT][5][64][4]      l_last^T of output tile m, K = 9 taps x 4 = 36 in 18 steps (20 stored): step s, lane l:
//                                       W3[tap = s>>1][c = 32 m + (l&31)][j = 2 (s&1) + (l>>5)]; the B operand is d(shift, raw)[j] at
//                                       pixel - (tap - centre)
//               A2T [MT][WP/8][64][4]   l_2^T of output tile m: K step kk = 4 kc + s consumes tile kk / 16, register kk % 16 of d h2:
//                                       lane l: W2[in = 32 m + (l&31)][out = 32 (kk/16) + c(kk%16, l>>5)]
//               A1T [MT][4][64][4]      l_1^T as D18 = W1 d h1: row i = l&31 = 2 tap + ch (18 used), step v of input tile mi:
//                                       W1[tap][ch][32 mi + c(v, l>>5)]
// Geometry of nf_gemm_kernel: bands of NB = 32768 / WP pixels, 512 threads, the band's activations ([WP][NB], 128 KiB) in LDS in
// B-operand order — h1 in the forward chain, the gated d h2 in the transposed one.  The partial D18 records of the WM = WP / 64
// wavefronts along the channel axis meet in the same region: NFGG_D_STRIDE floats per pixel, [2 tap + ch].
// Gate record: the sign of every D register of h1 (layer 0) and h2 (layer 1), 16 bits per lane and tile, in DEVICE SCRATCH per
// workgroup: uint16 [coupling][band][layer][tile = 32 of (m, nt)][lane] = 8 KiB per coupling and band — 2 WP bits per pixel.
// On gradient tiles (NF_CFG_GRAD_TILED_GEMM, the TILED instantiations) a launch is one segment on min(H,32) x min(W,32) tiles: the
// record of a workgroup then holds the couplings of the call's largest SEGMENT on one tile, the same function below sizing it.
#define NFGG_CPL_E 0
#define NFGG_CPL_S 64
#define NFGG_CPL_FWD 68
#define NFGG_D_STRIDE 20
#define NFGG_MAX_COUPLINGS 32   // couplings per model on this path: the scratch of a 32x32 patch at width 512 stays at 4 MiB per workgroup
__host__ __device__ constexpr int nfgg_cpl_bwd(int wp) { return 68 + (wp / 32) * 832 + wp * wp + (wp / 32) * (1024 + 128); }
__host__ __device__ constexpr int nfgg_bwd_A3T(int) { return 0; }
__host__ __device__ constexpr int nfgg_bwd_A2T(int wp) { return (wp / 32) * 1280; }
__host__ __device__ constexpr int nfgg_bwd_A1T(int wp) { return (wp / 32) * 1280 + wp * wp; }
__host__ __device__ constexpr int nfgg_bwd_size(int wp) { return (wp / 32) * (1280 + 1024) + wp * wp; }
__host__ __device__ constexpr int nfgg_cpl_size(int wp) { return nfgg_cpl_bwd(wp) + nfgg_bwd_size(wp); }
__host__ __device__ constexpr int nfgg_bands(int hw, int wp) { return (hw + 32768 / wp - 1) / (32768 / wp); }
// uint16 words of gate record per workgroup (one patch at a time): [coupling][band][2][32][64]
__host__ __device__ constexpr size_t nfgg_gate_halves(int hw, int wp, int n_cpl) { return (size_t)n_cpl * (size_t)nfgg_bands(hw, wp) * 4096; }
// LDS: the band, the zero-bordered tiles of z0 (2 planes) and d(shift, raw) (4 planes) at pitch W + 2, the reduction scratch
__host__ __device__ constexpr int nfgg_plane(int H, int W) { return ((H + 2) * (W + 2) + 3) & ~3; }
__host__ __device__ constexpr size_t nfgg_lds_floats(int H, int W) { return 32768 + 6 * (size_t)nfgg_plane(H, W) + 32; }
