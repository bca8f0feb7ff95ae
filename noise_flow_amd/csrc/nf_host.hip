// Host side of the C ABI (include/noiseflow_hip.h): parameter folding, program
// construction, conditioning scalars, launches.  No torch, no Python here.
//
// Reference call sites replaced (paths relative to /root/reference):
//   matrix_param.py:100-140      PLU -> A, A^-1, log|det|        (fold_conv1x1)
//   layers.py:378-401            BN eval folded into l_1 / l_2    (fold_coupling)
//   layers.py:555-583,651-674    edge channel + exp(3*logs)       (fold_coupling)
//   cond_utils.py:205-239        sdn5 scalars                     (nf_layers.h: nf_sdn_eval)
//   cond_utils.py:432-440        gain4                            (build_program)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/noiseflow_hip.h"
#include "nf_device.h"
#include "nf_gemm_layout.h"
#include "nf_internal.h"
#include "nf_layers.h"

hipError_t nf_launch_flow(const NfProgram &prog, const NfLaunch &a, int n_cu, hipStream_t stream, bool matrix_core, const float *block12 = nullptr,
                          size_t n_block12 = 0);
void nf_find_run(const NfProgram &prog, const float *block12, size_t n_block12, NfLaunch &a);
hipError_t nf_launch_wide(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
hipError_t nf_launch_wide16(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
hipError_t nf_launch_gemm(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
hipError_t nf_launch_gemm16(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
hipError_t nf_launch_gemm16b(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
bool nf_gemm_shape_ok(int H, int W);
hipError_t nf_launch_gemmb(const NfProgram &prog, const NfLaunch &a, int n_cu, int device, hipStream_t stream);
bool nf_gemmb_shape_ok(int wp, int H, int W);
bool nf_gemm16b_shape_ok(int wp, int H, int W);
hipError_t nf_launch_synth(uint64_t seed, int64_t patch_base, int64_t B, int HW, float beta1, float beta2,
                           float *y_out, float *x_out, hipStream_t stream);
hipError_t nf_launch_eps(uint64_t seed, int64_t patch_base, int64_t B, int HW, float *eps_out, hipStream_t stream);
hipError_t nf_launch_stats_compact(const double *stats, int nvals, double *buf, hipStream_t stream);
hipError_t nf_launch_stats_scatter(double *stats, int nvals, const double *buf, hipStream_t stream);
hipError_t nf_launch_sums_reduce(const double *wide, double *out3, bool accumulate, hipStream_t stream);
hipError_t nf_launch_bs_finalize(double *stats, int w, double n, float *Wm, int rows, float *Bv, float *mean_out, float *var_out,
                                 hipStream_t stream);
hipError_t nf_launch_tile_combine(const float *part, const NfTileParts &tp, int64_t B, double n, double ld_const, const nf_cond_row *cond_rows,
                                  uint32_t flags,
                                  float *nll_out, float *sd_out, float *ld_out, double *sums, hipStream_t stream);
// (the gradient kernels' launchers: nf_internal.h)

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    return fail(NF_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// ---- Conv2d1x1 (matrix_param.py): the matrices come from nf_layers.h, the inverses are formed as the reference forms them
void fold_conv1x1(const float *p, Mat4 &A, Mat4 &Ainv, double &log_abs_det)
{
    Mat4 Pm, L, U;
    log_abs_det = nf_plu_matrices(p, Pm, L, U);
    nf_plu_product(Pm, L, U, &A.m[0][0]);
    // A^-1 = U^-1 L^-1 P^T by two triangular solves (matrix_param.py:132-136)
    Mat4 X;   // X = L^-1 P^T  (forward substitution, unit diagonal)
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 4; ++i) {
            double s = Pm.m[c][i];   // P^T[i][c]
            for (int k = 0; k < i; ++k) s -= L.m[i][k] * X.m[k][c];
            X.m[i][c] = s;
        }
    for (int c = 0; c < 4; ++c)      // back substitution with U
        for (int i = 3; i >= 0; --i) {
            double s = X.m[i][c];
            for (int k = i + 1; k < 4; ++k) s -= U.m[i][k] * Ainv.m[k][c];
            Ainv.m[i][c] = s / U.m[i][i];
        }
}

// decomp = 'LU2': A^-1 = U^-1 L^-1 P^-1 from the three separate inverses, as the reference forms it (matrix_param.py:177-180)
bool fold_conv1x1_lu2(const float *p, Mat4 &A, Mat4 &Ainv, double &log_abs_det)
{
    Mat4 Pm, L, U, Pi, Li, Ui;
    log_abs_det = nf_lu2_matrices(p, Pm, L, U);
    nf_plu_product(Pm, L, U, &A.m[0][0]);
    double d;
    if (!nf_invert4(Pm, Pi, d) || !nf_invert4(L, Li, d) || !nf_invert4(U, Ui, d)) return false;
    Ainv = nf_matmul(Ui, nf_matmul(Li, Pi));
    return true;
}

// ---- coupling CNN folding ---------------------------------------------------
// `w` = width of the variables, `wk` >= w = width (and strides) of the block written: `out` arrives zeroed, the hidden channels
// w .. wk-1 keep zero weights and zero bias
void fold_coupling(const float *p, int w, int wk, float *out)
{
    const CplOff o = cpl_off(0, w);
    const float *W1 = p + o.w1, *b1 = p + o.b1, *m1 = p + o.m1, *v1 = m1 + w;
    const float *W2 = p + o.w2, *b2 = p + o.b2, *m2 = p + o.m2, *v2 = m2 + w;
    const float *W3 = p + o.w3;          // [3][3][w+1][4]
    const float *b3 = p + o.tail3, *logs = b3 + 4, *resc = logs + 4;

    std::vector<double> s1(w), s2(w);
    for (int j = 0; j < w; ++j) {
        s1[j] = 1.0 / sqrt((double)v1[j] + kBnEps);
        s2[j] = 1.0 / sqrt((double)v2[j] + kBnEps);
    }
    double es[4];
    for (int j = 0; j < 4; ++j) es[j] = exp(kLogscaleFactor * (double)logs[j]);

    float *E = out + nf_cpl_off_E(wk);
    for (int mask = 0; mask < 16; ++mask) {
        const bool top = mask & 1, bottom = mask & 2, left = mask & 4, right = mask & 8;
        for (int j = 0; j < 4; ++j) {
            double s = b3[j];
            for (int di = 0; di < 3; ++di)
                for (int dj = 0; dj < 3; ++dj) {
                    const bool outside = (di == 0 && top) || (di == 2 && bottom) || (dj == 0 && left) || (dj == 2 && right);
                    if (outside) s += (double)W3[((di * 3 + dj) * (w + 1) + w) * 4 + j];
                }
            E[mask * 4 + j] = (float)(s * es[j]);
        }
    }
    float *W3o = out + nf_cpl_off_W3(wk);
    for (int tap = 0; tap < 9; ++tap)
        for (int i = 0; i < w; ++i)
            for (int j = 0; j < 4; ++j)
                W3o[(tap * wk + i) * 4 + j] = (float)((double)W3[(tap * (w + 1) + i) * 4 + j] * es[j]);
    float *W1o = out + nf_cpl_off_W1(wk);
    for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < w; ++j)
                W1o[(tap * 2 + c) * wk + j] = (float)((double)W1[(tap * 2 + c) * w + j] * s1[j]);
    float *B1o = out + nf_cpl_off_B1(wk);
    for (int j = 0; j < w; ++j) B1o[j] = (float)(((double)b1[j] - (double)m1[j]) * s1[j]);
    float *W2o = out + nf_cpl_off_W2(wk);
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < w; ++j) W2o[i * wk + j] = (float)((double)W2[i * w + j] * s2[j]);
    float *B2o = out + nf_cpl_off_B2(wk);
    for (int j = 0; j < w; ++j) B2o[j] = (float)(((double)b2[j] - (double)m2[j]) * s2[j]);
    float *S = out + nf_cpl_off_S(wk);
    S[0] = resc[0];
    S[1] = S[2] = S[3] = 0.0f;
}

constexpr double kLog2e = 1.4426950408889634, k2Log2e = 2.0 * kLog2e;

// What every re-layout opens with: the border table E (16 masks x 4 channels) with 2*log2(e) folded into its raw columns, which
// feed exp2() directly, and the four scalars S of a generic coupling block of width `w`.
void relayout_ES(const float *v1, int w, float *E, float *S)
{
    for (int m = 0; m < 16; ++m)
        for (int j = 0; j < 4; ++j) {
            const float e = v1[nf_cpl_off_E(w) + 4 * m + j];
            E[4 * m + j] = j >= 2 ? (float)((double)e * k2Log2e) : e;
        }
    const double sc = v1[nf_cpl_off_S(w)];
    S[0] = (float)sc;
    S[1] = (float)(sc * kLog2e);          // scl:   ls*log2(e) = scl*tanh(raw)
    S[2] = (float)(-2.0 * sc * kLog2e);   // -2*scl
    S[3] = 0.0f;
}

// The two bias tables of the families that hold 32 hidden channels per tile (register v of lane half g = channel base +
// nf4_chan(v, g)); channels beyond the model's width `w` are zero.
void bias_tables32(const float *B1, const float *B2, int base, int w, float *o1, float *o2)
{
    for (int g = 0; g < 2; ++g)
        for (int v = 0; v < 16; ++v) {
            const int ch = base + nf4_chan(v, g);
            o1[g * 16 + v] = ch < w ? B1[ch] : 0.0f;
            o2[g * 16 + v] = ch < w ? B2[ch] : 0.0f;
        }
}

// The same folded coupling block re-laid out j-major for the matrix-core kernel
// (nf_device.h, NF2_CPL_*), width 4 only.
void relayout_coupling_v2(const float *v1, float *out)
{
    const int w = 4;
    const double k2 = k2Log2e;
    relayout_ES(v1, w, out + NF2_CPL_E, out + NF2_CPL_S);
    memcpy(out + NF2_CPL_B1, v1 + nf_cpl_off_B1(w), 4 * sizeof(float));
    memcpy(out + NF2_CPL_B2, v1 + nf_cpl_off_B2(w), 4 * sizeof(float));
    for (int j = 0; j < 4; ++j) {
        for (int di = 0; di < 3; ++di)
            for (int q = 0; q < 8; ++q)
                out[NF2_CPL_W1T + 24 * j + 8 * di + q] = q < 6 ? v1[nf_cpl_off_W1(w) + (di * 6 + q) * 4 + j] : 0.0f;
        for (int i = 0; i < 4; ++i) out[NF2_CPL_W2T + 4 * j + i] = v1[nf_cpl_off_W2(w) + i * 4 + j];
        for (int k = 0; k < 36; ++k) {
            const double wv = v1[nf_cpl_off_W3(w) + k * 4 + j];
            out[NF2_CPL_W3T + 36 * j + k] = (float)(j >= 2 ? wv * k2 : wv);
        }
    }
}

// fp16-CNN re-layout (nf_device.h, NF3_CPL_*): folded weights rounded to IEEE half.
uint16_t to_half(float f)
{
    _Float16 h = (_Float16)f;   // round-to-nearest-even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// l_last weights of the fp16-CNN layouts: output channel j of 4 = (shift, shift, raw, raw).  The raw columns carry the 2 log2(e)
// of  t = exp2(2 log2(e) raw) = exp(2 raw)  INSIDE the rounded weight — folded before the rounding to half, like the batch-norm
// scale and exp(3 logs) — so that no kernel multiplies behind its matrix instructions (oracle/nf_oracle.py::coupling_cnn_fp16
// rounds at the same point).
uint16_t to_half_w3(float wv, int j)
{
    _Float16 h = (_Float16)(j >= 2 ? (double)wv * k2Log2e : (double)wv);
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

void relayout_coupling_v3(const float *v1, float *out)
{
    const int w = 4;
    relayout_ES(v1, w, out + NF3_CPL_E, out + NF3_CPL_S);
    memcpy(out + NF3_CPL_B1, v1 + nf_cpl_off_B1(w), 4 * sizeof(float));
    memcpy(out + NF3_CPL_B2, v1 + nf_cpl_off_B2(w), 4 * sizeof(float));
    uint16_t *h1 = reinterpret_cast<uint16_t *>(out + NF3_CPL_W1H);
    uint16_t *h2 = reinterpret_cast<uint16_t *>(out + NF3_CPL_W2H);
    uint16_t *h3 = reinterpret_cast<uint16_t *>(out + NF3_CPL_W3H);
    auto W1 = [&](int di, int dj, int c, int j) { return to_half(v1[nf_cpl_off_W1(w) + ((di * 3 + dj) * 2 + c) * 4 + j]); };
    for (int j = 0; j < 4; ++j) {
        for (int di = 0; di < 3; ++di) {
            uint16_t *g = h1 + ((j * 3 + di) * 4) * 4;   // 4 groups x 4 halves
            const uint16_t z = 0;
            const uint16_t grp[4][4] = {
                {W1(di, 0, 0, j), W1(di, 0, 1, j), W1(di, 1, 0, j), W1(di, 1, 1, j)},   // dx=0, window pair (wc0,wc1)
                {W1(di, 2, 0, j), W1(di, 2, 1, j), z, z},                               // dx=0, pair (wc2,wc3)
                {z, z, W1(di, 0, 0, j), W1(di, 0, 1, j)},                               // dx=1, pair (wc0,wc1)
                {W1(di, 1, 0, j), W1(di, 1, 1, j), W1(di, 2, 0, j), W1(di, 2, 1, j)}};  // dx=1, pair (wc2,wc3)
            memcpy(g, grp, sizeof(grp));
        }
        for (int i = 0; i < 4; ++i) h2[j * 4 + i] = to_half(v1[nf_cpl_off_W2(w) + i * 4 + j]);
        for (int tap = 0; tap < 9; ++tap)
            for (int i = 0; i < 4; ++i) h3[j * (2 * NF3_W3H_STRIDE) + tap * 4 + i] = to_half_w3(v1[nf_cpl_off_W3(w) + (tap * 4 + i) * 4 + j], j);
    }
}

// fp16-CNN re-layout for v_mfma_f32_16x16x32_f16 (nf_device.h, NF11_*): the A operands in the order the lanes fetch them.
void relayout_coupling_v11(const float *v1, float *out, bool with_a2)
{
    const int w = 4;
    relayout_ES(v1, w, out + NF11_CPL_E, out + NF11_CPL_S);
    memcpy(out + NF11_CPL_B1, v1 + nf_cpl_off_B1(w), 4 * sizeof(float));
    memcpy(out + NF11_CPL_B2, v1 + nf_cpl_off_B2(w), 4 * sizeof(float));
    uint16_t *h2 = reinterpret_cast<uint16_t *>(out + NF11_CPL_W2H);
    uint16_t *a1 = reinterpret_cast<uint16_t *>(out + NF11_CPL_A1);
    uint16_t *a3 = reinterpret_cast<uint16_t *>(out + NF11_CPL_A3);
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) h2[j * 4 + i] = to_half(v1[nf_cpl_off_W2(w) + i * 4 + j]);
    auto tap_ok = [](int d) { return d >= 0 && d <= 2; };
    for (int l = 0; l < 64; ++l) {
        const int gk = l >> 4, m = l & 15, a = m >> 3, p = (m >> 2) & 1, j = m & 3;
        for (int e = 0; e < 8; ++e) {
            {   // l_1: element e = 2 wc + c of window row nf11_l1_row(gk)
                const int wc = e >> 1, c = e & 1, di = nf11_l1_row(gk) - a, dj = wc - p;
                a1[l * 8 + e] = tap_ok(di) && tap_ok(dj) ? to_half(v1[nf_cpl_off_W1(w) + ((di * 3 + dj) * 2 + c) * 4 + j]) : (uint16_t)0;
            }
            for (int m3 = 0; m3 < 2; ++m3) {   // l_last: element e = 4 px + c of window row nf11_l3_row(gk, m3), column pair gk >> 1
                const int wc = 2 * (gk >> 1) + (e >> 2), c = e & 3, di = nf11_l3_row(gk, m3) - a, dj = wc - p;
                a3[(m3 * 64 + l) * 8 + e] = tap_ok(di) && tap_ok(dj) ? to_half_w3(v1[nf_cpl_off_W3(w) + ((di * 3 + dj) * 4 + c) * 4 + j], j) : (uint16_t)0;
            }
        }
    }
    if (with_a2) {   // l_2 on the same instruction (nf_device.h, NF11_CPL_A2): block-diagonal over the lane's own K slot
        uint16_t *a2 = reinterpret_cast<uint16_t *>(out + NF11_CPL_A2);
        for (int half = 0; half < 2; ++half)
            for (int l = 0; l < 64; ++l) {
                const int gk = l >> 4, m = l & 15, g = m >> 2, j = m & 3;
                for (int e = 0; e < 8; ++e)
                    a2[(half * 64 + l) * 8 + e] = (gk == g && (e >> 2) == half) ? to_half(v1[nf_cpl_off_W2(w) + (e & 3) * 4 + j]) : (uint16_t)0;
            }
    }
}

// split-bf16 re-layout (nf_device.h, NF12_*): v = p[0] + p[1] + p[2], each piece the round-to-nearest-even bf16 of what the pieces
// before it left (the same split the kernel applies to its activations; every subtraction is exact in fp32)
void split_bf16x3_host(float v, uint16_t (&p)[3])
{
    float r = v;
    for (int q = 0; q < 3; ++q) {
        uint32_t u;
        memcpy(&u, &r, 4);
        const uint32_t hb = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;   // finite values only (folded weights)
        p[q] = (uint16_t)hb;
        const uint32_t back = hb << 16;
        float f;
        memcpy(&f, &back, 4);
        r -= f;
    }
}

// The LDS part of a coupling (E, B1, B2, S, W2t: the fp32 values of NF2_*) and its A image (l_1 / l_last weights split into three
// bf16 pieces, in the order the lanes of v_mfma_f32_16x16x32_bf16 fetch them).  AOFF is filled in by the caller.
void relayout_coupling_v12(const float *v1, float *lds, uint32_t *img)
{
    std::vector<float> v2(NF2_CPL_SIZE);
    relayout_coupling_v2(v1, v2.data());   // the exact-fp32 kernel's values: E and W3 carry 2 log2(e) in their raw columns
    memcpy(lds + NF12_CPL_E, v2.data() + NF2_CPL_E, 64 * sizeof(float));
    memcpy(lds + NF12_CPL_B1, v2.data() + NF2_CPL_B1, 4 * sizeof(float));
    memcpy(lds + NF12_CPL_B2, v2.data() + NF2_CPL_B2, 4 * sizeof(float));
    memcpy(lds + NF12_CPL_S, v2.data() + NF2_CPL_S, 4 * sizeof(float));
    memcpy(lds + NF12_CPL_W2T, v2.data() + NF2_CPL_W2T, 16 * sizeof(float));
    for (int q = NF12_CPL_AOFF; q < NF12_CPL_SIZE; ++q) lds[q] = 0.0f;
    uint16_t *a1 = reinterpret_cast<uint16_t *>(img + NF12_A_A1);
    uint16_t *a3 = reinterpret_cast<uint16_t *>(img + NF12_A_A3);
    auto tap_ok = [](int d) { return d >= 0 && d <= 2; };
    for (int l = 0; l < 64; ++l) {
        const int gk = l >> 4, m = l & 15, a = m >> 3, p = (m >> 2) & 1, j = m & 3;
        for (int e = 0; e < 8; ++e) {
            for (int half = 0; half < 2; ++half) {   // l_1: window row nf11_l1_row(gk), column 2 half + (e >> 2), slot word (e >> 1) & 1
                const int wc = 2 * half + (e >> 2), ws = (e >> 1) & 1, c = e & 1, di = nf11_l1_row(gk) - a, dj = wc - p;
                uint16_t pc[3] = {0, 0, 0};
                if (tap_ok(di) && tap_ok(dj)) split_bf16x3_host(v2[NF2_CPL_W1T + 24 * j + 8 * di + 2 * dj + c], pc);
                const uint16_t pick[3] = {pc[0], pc[1], ws == 0 ? pc[0] : pc[2]};   // pairs (h | h), (m | m), (h | l)
                for (int pr = 0; pr < 3; ++pr) a1[((pr * 2 + half) * 64 + l) * 8 + e] = pick[pr];
            }
            for (int m3 = 0; m3 < 2; ++m3) {   // l_last: as NF11 (element e = 4 px + c of window row nf11_l3_row(gk, m3), column pair gk >> 1)
                const int wc = 2 * (gk >> 1) + (e >> 2), c = e & 3, di = nf11_l3_row(gk, m3) - a, dj = wc - p;
                uint16_t pc[3] = {0, 0, 0};
                if (tap_ok(di) && tap_ok(dj)) split_bf16x3_host(v2[NF2_CPL_W3T + 36 * j + (di * 3 + dj) * 4 + c], pc);
                for (int q = 0; q < 3; ++q) a3[((q * 2 + m3) * 64 + l) * 8 + e] = pc[q];
            }
        }
    }
}

// Wide-CNN re-layout (nf_device.h, NF4_*; coupling width 32): every weight in the order the lanes of
// v_mfma_f32_32x32x2_f32 / v_mfma_f32_4x4x1 fetch their A operands (nf_wide.hip).
// `w` = the coupling's own width (8, 16 or 32): narrower CNNs are zero-padded to 32 hidden channels (exact: a padded
// channel has zero weights and zero bias in l_1 / l_2, hence zero activation, and zero l_last weights).
void relayout_coupling_wide32(const float *v1, int w, float *out)
{
    const double k2 = k2Log2e;
    relayout_ES(v1, w, out + NF4_CPL_E, out + NF4_CPL_S);
    float *img = out + NF4_CPL_IMG;
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    for (int step = 0; step < 12; ++step)          // l_1: step = tap, K slice = input channel
        for (int l = 0; l < 64; ++l)
            img[NF4_IMG_A1 + ((step >> 2) * 64 + l) * 4 + (step & 3)] =
                (step < 9 && (l & 31) < w) ? W1[(step * 2 + (l >> 5)) * w + (l & 31)] : 0.0f;
    bias_tables32(B1, B2, 0, w, img + NF4_IMG_B1, img + NF4_IMG_B2);
    // taps (di,dj) of the 8 off-centre rows groups of P, by (a, g')
    static const int tap_of[4][2] = {{0 * 3 + 0, 2 * 3 + 0}, {0 * 3 + 2, 2 * 3 + 2}, {0 * 3 + 1, 2 * 3 + 1}, {1 * 3 + 0, 1 * 3 + 2}};
    for (int s = 0; s < 16; ++s)
        for (int l = 0; l < 64; ++l) {
            const int cin = nf4_chan(s, l >> 5), i = l & 31;
            img[NF4_IMG_A2 + ((s >> 2) * 64 + l) * 4 + (s & 3)] = (cin < w && i < w) ? W2[cin * w + i] : 0.0f;
            const int a = i >> 3, gp = (i >> 2) & 1, j = i & 3;
            const double wv = cin < w ? W3[(tap_of[a][gp] * w + cin) * 4 + j] : 0.0;
            img[NF4_IMG_A3 + ((s >> 2) * 64 + l) * 4 + (s & 3)] = (float)(j >= 2 ? wv * k2 : wv);
        }
    for (int s = 0; s < 16; ++s)
        for (int g = 0; g < 2; ++g)
            for (int j = 0; j < 4; ++j) {
                const double wv = nf4_chan(s, g) < w ? W3[(4 * w + nf4_chan(s, g)) * 4 + j] : 0.0;   // centre tap (1,1)
                img[NF4_IMG_A3C + ((s >> 2) * 8 + g * 4 + j) * 4 + (s & 3)] = (float)(j >= 2 ? wv * k2 : wv);
            }
}

// GEMM re-layout (nf_device.h, NF7_*; widths 33 .. 512 zero-padded to wp = 64 / 128 / 256 / 512): every weight in the order the
// wavefront that consumes it fetches it from L2 (nf_gemm.hip).
// the NF7 image (A1, B1, B2, A2, A3, A3C) with the raw columns of l_last scaled by k2: 2 log2(e) for the flow kernels, 1 for the
// gradient kernel (nf_gemm_layout.h, NFGG_*), which takes tanh / exp of unscaled values
void relayout_gemm_image(const float *v1, int w, int wp, double k2, float *img)
{
    const int MT = wp / 32, KC = wp / 8;
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    for (int m = 0; m < MT; ++m) {
        for (int step = 0; step < 12; ++step)          // l_1: step = tap, K slice = input channel
            for (int l = 0; l < 64; ++l) {
                const int oc = 32 * m + (l & 31);
                img[nf7_img_A1(wp) + ((m * 3 + (step >> 2)) * 64 + l) * 4 + (step & 3)] =
                    (step < 9 && oc < w) ? W1[(step * 2 + (l >> 5)) * w + oc] : 0.0f;
            }
        bias_tables32(B1, B2, 32 * m, w, img + nf7_img_B1(wp) + m * 32, img + nf7_img_B2(wp) + m * 32);
        for (int kc = 0; kc < KC; ++kc)                // l_2: K step kk = 4 kc + s consumes input tile kk / 16, register kk % 16
            for (int l = 0; l < 64; ++l)
                for (int s2 = 0; s2 < 4; ++s2) {
                    const int kk = 4 * kc + s2, cin = 32 * (kk / 16) + nf4_chan(kk % 16, l >> 5), oc = 32 * m + (l & 31);
                    img[nf7_img_A2(wp) + (((size_t)m * KC + kc) * 64 + l) * 4 + s2] = (cin < w && oc < w) ? W2[(size_t)cin * w + oc] : 0.0f;
                }
    }
    for (int mi = 0; mi < MT; ++mi)                    // P = W3^T h2: taps 0 .. 7 as one 32-row GEMM (row i = 4 tap + j) ...
        for (int v = 0; v < 16; ++v)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, cin = 32 * mi + nf4_chan(v, l >> 5);
                double wv = 0.0;
                if (cin < w) {
                    const int tap = row >> 2, j = row & 3;
                    wv = W3[((size_t)tap * w + cin) * 4 + j];
                    if (j >= 2) wv *= k2;
                }
                img[nf7_img_A3(wp) + (((size_t)mi * 4 + (v >> 2)) * 64 + l) * 4 + (v & 3)] = (float)wv;
            }
    for (int mi = 0; mi < MT; ++mi)                    // ... and tap 8 on v_mfma_f32_4x4x1 (4 rows, not a 32-row tile)
        for (int v = 0; v < 16; ++v)
            for (int g = 0; g < 2; ++g)
                for (int j = 0; j < 4; ++j) {
                    const int cin = 32 * mi + nf4_chan(v, g);
                    double wv = cin < w ? (double)W3[((size_t)8 * w + cin) * 4 + j] : 0.0;
                    if (j >= 2) wv *= k2;
                    img[nf7_img_A3C(wp) + (((size_t)mi * 4 + (v >> 2)) * 8 + g * 4 + j) * 4 + (v & 3)] = (float)wv;
                }
}
void relayout_coupling_gemm(const float *v1, int w, int wp, float *out)
{
    relayout_ES(v1, w, out + NF7_CPL_E, out + NF7_CPL_S);
    relayout_gemm_image(v1, w, wp, k2Log2e, out + NF7_CPL_IMG);
}

// Variant B of the GEMM layout (NF10_*, widths <= 128): the NF7 values, one contiguous slab per channel tile.
void relayout_coupling_gemmb(const float *v1, int w, int wp, float *out)
{
    std::vector<float> a(nf7_cpl_size(wp));
    relayout_coupling_gemm(v1, w, wp, a.data());
    const int MT = wp / 32, KC = wp / 8;
    memcpy(out, a.data(), (size_t)(NF7_CPL_IMG + MT * 832) * sizeof(float));      // E, S, A1, B1 (+ NF7's B2 block, unused)
    const float *ia = a.data() + NF7_CPL_IMG;
    float *io = out + NF7_CPL_IMG;
    for (int m = 0; m < MT; ++m) {
        float *sl = io + nf10_img_SLAB(wp) + (size_t)m * nf10_slab_floats(wp);
        memcpy(sl, ia + nf7_img_A2(wp) + (size_t)m * KC * 256, (size_t)KC * 256 * sizeof(float));
        memcpy(sl + nf10_slab_A3(wp), ia + nf7_img_A3(wp) + (size_t)m * 1024, 1024 * sizeof(float));
        memcpy(sl + nf10_slab_A3C(wp), ia + nf7_img_A3C(wp) + (size_t)m * 128, 128 * sizeof(float));
        memcpy(sl + nf10_slab_B2(wp), ia + nf7_img_B2(wp) + (size_t)m * 32, 32 * sizeof(float));
    }
}

// fp16-CNN GEMM re-layout (nf_gemm_layout.h, NF8_*; NF_CFG_FP16_CNN at widths 33 .. 512): fetch order of v_mfma_f32_32x32x16_f16,
// folded weights rounded to half once (the oracle's rounding points), biases / border table fp32.
void relayout_coupling_gemm16(const float *v1, int w, int wp, float *out)
{
    const int MT = wp / 32, KS = wp / 16;
    relayout_ES(v1, w, out + NF8_CPL_E, out + NF8_CPL_S);
    float *img = out + NF8_CPL_IMG;
    memset(img, 0, (size_t)nf8_img_size(wp) * sizeof(float));
    uint16_t *h = reinterpret_cast<uint16_t *>(img);   // half index = 2 * dword index
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    for (int m = 0; m < MT; ++m) {
        for (int l = 0; l < 64; ++l) {
            const int oc = 32 * m + (l & 31), g = l >> 5;
            for (int q = 0; q < 8; ++q) {
                // l_1, instruction 0: taps 4g .. 4g+3; instruction 1: tap 8 on lane half 0
                const int tap = 4 * g + (q >> 1), ch = q & 1;
                h[2 * ((size_t)nf8_img_A1H(wp) + ((m * 2 + 0) * 64 + l) * 4) + q] = oc < w ? to_half(W1[(tap * 2 + ch) * w + oc]) : 0;
                h[2 * ((size_t)nf8_img_A1H(wp) + ((m * 2 + 1) * 64 + l) * 4) + q] = (oc < w && g == 0 && q < 2) ? to_half(W1[(8 * 2 + q) * w + oc]) : 0;
                for (int ks = 0; ks < KS; ++ks) {
                    const int cin = 32 * (ks >> 1) + nf4_chan(8 * (ks & 1) + q, g);
                    h[2 * ((size_t)nf8_img_A2H(wp) + (((size_t)m * KS + ks) * 64 + l) * 4) + q] =
                        (cin < w && oc < w) ? to_half(W2[(size_t)cin * w + oc]) : 0;
                }
                for (int m2 = 0; m2 < 2; ++m2) {       // P rows of taps 0 .. 7 from INPUT tile m
                    const int cin = 32 * m + nf4_chan(8 * m2 + q, g), row = l & 31, tap = row >> 2, j = row & 3;
                    h[2 * ((size_t)nf8_img_A3H(wp) + ((m * 2 + m2) * 64 + l) * 4) + q] = cin < w ? to_half_w3(W3[((size_t)tap * w + cin) * 4 + j], j) : 0;
                }
            }
        }
        bias_tables32(B1, B2, 32 * m, w, img + nf8_img_B1(wp) + m * 32, img + nf8_img_B2(wp) + m * 32);
        for (int q4 = 0; q4 < 4; ++q4)                 // tap 8 on v_mfma_f32_4x4x4_16b_f16
            for (int g = 0; g < 2; ++g)
                for (int j = 0; j < 4; ++j)
                    for (int r = 0; r < 4; ++r) {
                        const int cin = 32 * m + nf4_chan(4 * q4 + r, g);
                        h[2 * ((size_t)nf8_img_A3CH(wp) + ((m * 4 + q4) * 8 + g * 4 + j) * 2) + r] =
                            cin < w ? to_half_w3(W3[((size_t)8 * w + cin) * 4 + j], j) : 0;
                    }
    }
}

// Variant B of the fp16-CNN GEMM layout (NF9_*): the same values, one contiguous slab per channel tile.
void relayout_coupling_gemm16b(const float *v1, int w, int wp, float *out)
{
    std::vector<float> a(nf8_cpl_size(wp));
    relayout_coupling_gemm16(v1, w, wp, a.data());
    const int MT = wp / 32, KS = wp / 16;
    memcpy(out, a.data(), (size_t)(NF8_CPL_IMG + MT * 544) * sizeof(float));      // E, S, A1H, B1 (same offsets)
    const float *ia = a.data() + NF8_CPL_IMG;
    float *io = out + NF8_CPL_IMG;
    for (int m = 0; m < MT; ++m) {
        float *sl = io + nf9_img_SLAB(wp) + (size_t)m * nf9_slab_dwords(wp);
        memcpy(sl, ia + nf8_img_A2H(wp) + (size_t)m * KS * 256, (size_t)KS * 256 * sizeof(float));
        memcpy(sl + nf9_slab_A3H(wp), ia + nf8_img_A3H(wp) + (size_t)m * 512, 512 * sizeof(float));
        memcpy(sl + nf9_slab_A3CH(wp), ia + nf8_img_A3CH(wp) + (size_t)m * 64, 64 * sizeof(float));
        memcpy(sl + nf9_slab_B2(wp), ia + nf8_img_B2(wp) + (size_t)m * 32, 32 * sizeof(float));
    }
}

// Width-16 re-layout (nf_device.h, NF6_*; `w` = 16, or 8 zero-padded): fetch order of v_mfma_f32_16x16x4_f32.
void relayout_coupling_wide16(const float *v1, int w, float *out)
{
    const double k2 = k2Log2e;
    relayout_ES(v1, w, out + NF4_CPL_E, out + NF4_CPL_S);
    float *img = out + NF4_CPL_IMG;
    memset(img, 0, NF6_IMG_SIZE * sizeof(float));
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    static const int tapA[4] = {0 * 3 + 0, 1 * 3 + 0, 2 * 3 + 0, 0 * 3 + 1}, tapB[4] = {0 * 3 + 2, 1 * 3 + 2, 2 * 3 + 2, 2 * 3 + 1};
    for (int l = 0; l < 64; ++l) {
        const int i = l & 15, g = l >> 4;
        for (int s = 0; s < 5; ++s) {
            const int kk = 4 * s + g;
            const float v = (kk < 18 && i < w) ? W1[kk * w + i] : 0.0f;   // kk = tap * 2 + ch
            if (s < 4) img[NF6_IMG_A1 + l * 4 + s] = v;
            else img[NF6_IMG_A1 + 256 + l] = v;
        }
        for (int s = 0; s < 4; ++s) {
            const int cin = 4 * g + s;
            img[NF6_IMG_A2 + l * 4 + s] = (cin < w && i < w) ? W2[cin * w + i] : 0.0f;
            const int gp = i >> 2, j = i & 3;
            const double wa = cin < w ? W3[(tapA[gp] * w + cin) * 4 + j] : 0.0, wb = cin < w ? W3[(tapB[gp] * w + cin) * 4 + j] : 0.0;
            img[NF6_IMG_A3A + l * 4 + s] = (float)(j >= 2 ? wa * k2 : wa);
            img[NF6_IMG_A3B + l * 4 + s] = (float)(j >= 2 ? wb * k2 : wb);
        }
    }
    for (int g = 0; g < 4; ++g)
        for (int v = 0; v < 4; ++v) {
            const int ch = 4 * g + v;
            img[NF6_IMG_B1 + g * 4 + v] = ch < w ? B1[ch] : 0.0f;
            img[NF6_IMG_B2 + g * 4 + v] = ch < w ? B2[ch] : 0.0f;
            for (int j = 0; j < 4; ++j) {   // here v plays the K step s
                const double wv = ch < w ? W3[(4 * w + ch) * 4 + j] : 0.0;
                img[NF6_IMG_A3C + (g * 4 + j) * 4 + v] = (float)(j >= 2 ? wv * k2 : wv);
            }
        }
}

// fp16 variant of the wide layout (nf_device.h, NF5_*): folded weights rounded to half, in the fetch order of
// v_mfma_f32_32x32x16_f16 (8 halves per lane and instruction) / v_mfma_f32_4x4x4_16b_f16 (centre tap).
void relayout_coupling_wide32_fp16(const float *v1, int w, float *out)
{
    relayout_ES(v1, w, out + NF4_CPL_E, out + NF4_CPL_S);
    float *img = out + NF4_CPL_IMG;
    memset(img, 0, NF5_IMG_SIZE * sizeof(float));
    uint16_t *h = reinterpret_cast<uint16_t *>(img);   // half index = 2 * dword index
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    static const int tap_of[4][2] = {{0 * 3 + 0, 2 * 3 + 0}, {0 * 3 + 2, 2 * 3 + 2}, {0 * 3 + 1, 2 * 3 + 1}, {1 * 3 + 0, 1 * 3 + 2}};
    for (int l = 0; l < 64; ++l) {
        const int i = l & 31, g = l >> 5;
        for (int q = 0; q < 8; ++q) {
            // l_1, instruction 0: taps 4g .. 4g+3; instruction 1: tap 8 on lane half 0
            const int tap = 4 * g + (q >> 1), ch = q & 1;
            h[2 * (NF5_IMG_A1H + (0 * 64 + l) * 4) + q] = i < w ? to_half(W1[(tap * 2 + ch) * w + i]) : 0;
            h[2 * (NF5_IMG_A1H + (1 * 64 + l) * 4) + q] = (i < w && g == 0 && q < 2) ? to_half(W1[(8 * 2 + q) * w + i]) : 0;
            for (int m = 0; m < 2; ++m) {
                const int cin = nf4_chan(8 * m + q, g);
                h[2 * (NF5_IMG_A2H + (m * 64 + l) * 4) + q] = (cin < w && i < w) ? to_half(W2[cin * w + i]) : 0;
                const int a = i >> 3, gp = (i >> 2) & 1, j = i & 3;
                h[2 * (NF5_IMG_A3H + (m * 64 + l) * 4) + q] = cin < w ? to_half_w3(W3[(tap_of[a][gp] * w + cin) * 4 + j], j) : 0;
            }
        }
    }
    bias_tables32(B1, B2, 0, w, img + NF5_IMG_B1, img + NF5_IMG_B2);
    for (int q = 0; q < 4; ++q)
        for (int g = 0; g < 2; ++g)
            for (int j = 0; j < 4; ++j)
                for (int r = 0; r < 4; ++r) {
                    const int cin = nf4_chan(4 * q + r, g);
                    h[2 * (NF5_IMG_A3CH + (q * 8 + g * 4 + j) * 2) + r] = cin < w ? to_half_w3(W3[(4 * w + cin) * 4 + j], j) : 0;   // centre tap
                }
}

// ---- per-call scalars of the conditional layers (formulas: nf_layers.h) ---------
struct CondLayer {
    int kind;                  // NF_LAYER_* of an sdn or conditional-gain kind
    std::vector<float> p;      // its raw parameters
};

inline bool is_gain_kind(int k) { return nf_layer_info(k).cls == NF_CLS_COND_GAIN; }

// Per-call scalars of one conditional layer -> (a, b): SDN kinds: scale^2 = a*y + b; GAIN: scale = a, and *K = how many
// log(scale) terms its log-det holds on patches of HW pixels.
int cond_scalars(int kind, const float *p, const nf_cond *cond, double out[2], int HW = 0, double *K = nullptr)
{
    const NfLayerInfo &info = nf_layer_info(kind);
    if (info.cls != NF_CLS_SDN && info.cls != NF_CLS_COND_GAIN) return fail(NF_EINVAL, "bad conditional layer");
    CondIdx ci{0.f, -1, 0};
    if (info.iso) {
        if (!cond) return fail(NF_EINVAL, "model has %s but cond is NULL", info.name);
        ci = nf_cond_index(cond);
        if (info.cam && ci.cam_idx < 0) return fail(NF_ECOND, NF_CAM_ERROR, (double)cond->cam);
    }
    if (info.cls == NF_CLS_SDN) {
        NfSdn s;
        nf_sdn_eval(kind, p, ci, s);
        out[0] = s.a;
        out[1] = s.b;
        return NF_OK;
    }
    double k;
    nf_gain_eval(kind, p, ci, HW, out[0], k);
    if (K) *K = k;
    out[1] = 0.0;
    if (kind != NF_LAYER_GAIN1 && !(out[0] > 0.0)) return fail(NF_EINVAL, "gain scale must be > 0");
    return NF_OK;
}

// ---- program construction -----------------------------------------------------
constexpr int NF_PATH_COUNT = 9;   // the NF_PATH_* values of noiseflow_hip.h index every per-family table of this file

struct Layout {
    NfProgram prog = {};
    std::vector<float> block;   // empty: the model has no such layout
};

struct Built {
    std::vector<CondLayer> cond;   // conditioning slots, in the order the ops reference them
    // One program + parameter block per kernel family, all the same op sequence:
    //   NF_PATH_SCALAR       the generic layout every other one is made from (always there)
    //   NF_PATH_MFMA4        matrix-core layout (NF2_*: j-major weights), width 4 only
    //   NF_PATH_SPLIT_BF16   NF12_*: width 4 in fp32 on full 32x32 patches unless NF_CFG_EXACT_FP32; the LDS part (n_lds9 floats),
    //                        then the couplings' A images
    //   NF_PATH_FP16         fp16-CNN layout (NF_CFG_FP16_CNN), width 4 only
    //   NF_PATH_WIDE32       wide-CNN layout (NF4_*), width 32 (8 / 16 zero-padded on large patches)
    //   NF_PATH_WIDE32_FP16  wide-CNN fp16 layout (NF5_*): NF_CFG_FP16_CNN at widths 8 / 16 / 32
    //   NF_PATH_WIDE16       width-16 layout (NF6_*)
    //   NF_PATH_GEMM         NF7_*: widths 33 .. 512, zero-padded to 64 / 128 / 256 / 512
    //   NF_PATH_GEMM_FP16    NF8_*: NF_CFG_FP16_CNN at widths 33 .. 512
    Layout lay[NF_PATH_COUNT];
    int n_lds9 = 0;
    bool fp16_big = false;       // the NF_PATH_FP16 block is the NF11_* layout (v_mfma_f32_16x16x32_f16) instead of NF3_* (4x4x4)
    int raw_width = 4;           // coupling width of the model's variables; lay[0].prog.width is the (zero-padded) width the kernels run
    bool gemm_b = false;         // the NF_PATH_GEMM block is in the variant-B layout (NF10_*: widths <= 128, weights resident in LDS)
    bool gemm16_b = false;       // the NF_PATH_GEMM_FP16 block is in the variant-B layout (NF9_*: widths <= 128)
    double ld_const = 0.0;
    bool has_sdn = false;      // some op reads the clean image y
    // images beyond 64x64 (nf_device.h, NF_K_TILED): the kernels run on overlapping tile_h x tile_w tiles, the program cut
    // into segments (ops [op0, op1) each, its own halo and tile counts)
    bool tiled = false;
    int tile_h = 0, tile_w = 0;
    struct TileSeg {
        int op0, op1, halo, ny, nx;
    };
    std::vector<TileSeg> segs;
};

// Cut a tiled program into segments (nf_device.h): the couplings dealt as evenly as possible to S consecutive groups, a
// segment ending right after its last coupling (the pointwise ops behind the last coupling stay with the last segment), S
// chosen for the least estimated work, in units of one coupling on one tile: tiles of a segment x (its couplings + 0.75 for the
// tile's load / store / set-up and the pointwise layers) + 1 per 4096 image pixels and segment boundary (32 B per pixel
// through HBM) — fitted to tools/time_large_patches.py at 256^2 and 1024^2.  NF_TILE_SEGMENTS=<n> forces S (A/B and test aid).
// The same planner cuts the program for the tiled gradient (NF_CFG_GRAD_TILED, nf_device.h "gradient tiles"): 32-pixel tiles, a
// halo of 4 per coupling, NF_GRAD_TILE_SEGMENTS.  Its constants are fitted to tools/time_nll_grad.py --legs tiled
// (profiles/nll_grad_tiled.txt: the shipped model at 256^2 x 16 and 1024^2 x 1, S = 8 / 4 / 3, six timings): least squares over
// (tile-couplings, tiles, boundary pixels) gives 17.9 ns per tile-coupling, 31.0 ns per tile and -0.003 ns per boundary pixel —
// no boundary cost these runs can resolve, so the term is 0 — and over the first two alone 18.5 ns and 29.1 ns (residuals within
// 3.1 %): a tile costs its couplings + 1.57.  One coupling per segment wins on every image of more than a few tiles.
// Width 32 on tiles (NF_CFG_GRAD_TILED_WIDE, nf_grad_wide_kernel<.., TILED>) has a rule of its own, kGradWideSegs: the same tiles,
// halo and switch, at most 3 couplings per segment on a single tile too.  Its per-tile constant is the scalar kernel's 1.57: with it
// the unforced plan is the fastest measured arm (tools/time_nll_grad.py --legs tiled_wide, profiles/nll_grad_tiled_wide.txt: width 32
// x 8 couplings at 256^2 x 16 and 64^2 x 1 024, unforced and S = 8 / 4 / 3), which is what keeps it.  Least squares over the six forced
// arms gives 199.6 ns per tile-coupling and -6.3 ns per tile with residuals up to 21 %: a tile of a 3-coupling segment costs more than
// three one-coupling tiles (80.6 KiB of LDS: one workgroup per CU instead of two), which two terms cannot say.
// Widths 33 .. 512 on tiles (NF_CFG_GRAD_TILED_GEMM, nf_grad_gemm_kernel<.., TILED>): kGradGemmSegs, the same tiles, halo, switch and
// limit of 3 couplings per segment.  Its per-tile constant is measured (tools/time_nll_grad.py --legs tiled_gemm,
// profiles/nll_grad_tiled_gemm.txt: 8 couplings at widths 64 / 128 / 512 on 64^2 x 256 and 256^2 x 16, unforced and S = 8 .. 3): least
// squares over the twelve forced arms of a width gives 558 / 1 369 / 13 420 ns per tile-coupling and 205 / 544 / 5 103 ns per tile — a
// tile costs its couplings + 0.37 / 0.40 / 0.38 at the three widths (residuals up to 16 %: the launches of 256^2 x 16 fill the 256
// CUs less evenly than those of 64^2 x 256, which two terms cannot say), no boundary cost these runs resolve.  With 0.38 the unforced
// plan is the fastest measured arm, or within the spread of the repeated timings of it, at every width and on both workloads.
struct SegRule {
    const char *env;       // forces S
    int tile;              // tile side the core must fit
    int halo_per_cpl;
    double per_tile;       // cost of a tile beside its couplings, in tile-couplings
    double per_boundary_px;   // cost of one image pixel of a segment boundary, in tile-couplings
    const char *what;
    int max_cpl = 0;       // most couplings of a segment whatever the tile count (0: no such limit)
};
static const SegRule kFwdSegs = {"NF_TILE_SEGMENTS", 64, 2, 0.75, 1.0 / 4096.0, "patches beyond 64x64"};
static const SegRule kGradSegs = {"NF_GRAD_TILE_SEGMENTS", NF_GRAD_TILE, 4, 1.57, 0.0, "nf_nll_grad on tiles"};
static const SegRule kGradWideSegs = {"NF_GRAD_TILE_SEGMENTS", NF_GRAD_TILE, 4, 1.57, 0.0, "nf_nll_grad on tiles at coupling width 32", 3};   // 3: the gate record of a 32x32 tile beside the rest, and 32 - 2 x 12 = 8 core pixels
static const SegRule kGradGemmSegs = {"NF_GRAD_TILE_SEGMENTS", NF_GRAD_TILE, 4, 0.38, 0.0, "nf_nll_grad on tiles at coupling widths beyond 32", 3};   // 3: 32 - 2 x 12 = 8 core pixels
static int plan_tile_segments(const NfProgram &prog, int H, int W, int th, int tw, std::vector<Built::TileSeg> &segs, const SegRule &rule = kFwdSegs)
{
    std::vector<int> cpl;
    for (int i = 0; i < prog.n_ops; ++i)
        if (prog.ops[i].type == NF_OP_COUPLING_FWD || prog.ops[i].type == NF_OP_COUPLING_REV) cpl.push_back(i);
    const int n_cpl = (int)cpl.size();
    const char *e = getenv(rule.env);
    const int forced = e ? atoi(e) : 0;
    double best = 0.0;
    segs.clear();
    const int s_max = n_cpl < 1 ? 1 : n_cpl < NF_MAX_TILE_SEGS ? n_cpl : NF_MAX_TILE_SEGS;
    const int s_only = forced > 0 ? (forced < s_max ? forced : s_max) : 0;
    for (int S = 1; S <= s_max; ++S) {
        if (s_only && S != s_only) continue;
        std::vector<Built::TileSeg> cand;
        double cost = 0.0;
        bool ok = true;
        int c0 = 0, op0 = 0;
        for (int sgm = 0; sgm < S; ++sgm) {
            const int nc = n_cpl / S + (sgm < n_cpl % S ? 1 : 0);
            Built::TileSeg t;
            t.op0 = op0;
            t.op1 = sgm == S - 1 ? prog.n_ops : cpl[c0 + nc - 1] + 1;
            t.halo = rule.halo_per_cpl * nc;
            if ((H > th || W > tw) && rule.tile - 2 * t.halo < 8) ok = false;   // no core left in a tile
            if (rule.max_cpl && nc > rule.max_cpl) ok = false;
            if (!ok) break;
            t.ny = nf_tile_count(H, th, t.halo);
            t.nx = nf_tile_count(W, tw, t.halo);
            cost += (double)t.ny * t.nx * (nc + rule.per_tile);
            if (sgm > 0) cost += (double)H * W * rule.per_boundary_px;   // the tensor between two segments (forward: one tile-coupling per 4096 pixels; x 2^-12 is exact)
            cand.push_back(t);
            c0 += nc;
            op0 = t.op1;
        }
        if (!ok) continue;
        if (segs.empty() || cost < best) {
            best = cost;
            segs.swap(cand);
        }
    }
    if (segs.empty()) return fail(NF_EINVAL, "%s: %d coupling layers cannot be cut into at most %d tiled segments", rule.what, n_cpl, NF_MAX_TILE_SEGS);
    return NF_OK;
}

// One family's program and block from the generic ones — the same op sequence: a 1x1 matrix copied, or stored transposed
// (`mix_t`: j-major, the width-4 matrix-core kernels), `cpl_floats` reserved per coupling and filled by
// relayout(the coupling's generic block, its place in the new block), a scale copied, a conditioning slot passed through.
template <class Relayout>
void build_layout(const Layout &gen, Layout &out, int width, bool mix_t, size_t cpl_floats, Relayout relayout)
{
    out.prog.width = width;
    for (int i = 0; i < gen.prog.n_ops; ++i) {
        const NfOp &src = gen.prog.ops[i];
        NfOp &dst = out.prog.ops[out.prog.n_ops++];
        dst.type = src.type;
        dst.off = (int32_t)out.block.size();
        const float *v1 = gen.block.data() + src.off;
        if (src.type == NF_OP_MIX) {
            for (int q = 0; q < 16; ++q) out.block.push_back(mix_t ? v1[(q & 3) * 4 + (q >> 2)] : v1[q]);
        } else if (src.type == NF_OP_COUPLING_FWD || src.type == NF_OP_COUPLING_REV) {
            out.block.resize(out.block.size() + cpl_floats);
            relayout(v1, out.block.data() + dst.off);
        } else if (src.type == NF_OP_SCALE) {
            out.block.insert(out.block.end(), v1, v1 + 4);
        } else {
            dst.off = src.off;   // conditioning slot
        }
    }
    if (out.block.empty()) out.block.assign(4, 0.0f);
}

int build_program(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params,
                  int direction, Built &out)
{
    if (!cfg || !layers || !params) return fail(NF_EINVAL, "null argument");
    if (cfg->channels != kC) return fail(NF_EINVAL, "channels must be 4 (packed raw), got %d", cfg->channels);
    if (cfg->height < 1 || cfg->width < 1 || cfg->height > NF_MAX_IMAGE_SIDE || cfg->width > NF_MAX_IMAGE_SIDE)
        return fail(NF_EINVAL, "patch size %dx%d unsupported (1 .. %d per side)", cfg->height, cfg->width, NF_MAX_IMAGE_SIDE);
    // one workgroup holds up to 64x64 pixels; larger images are evaluated as overlapping tiles of th x tw pixels, and every
    // kernel-shape decision below is about the tile
    const int th = cfg->height < 64 ? cfg->height : 64, tw = cfg->width < 64 ? cfg->width : 64;
    out.tiled = cfg->height > 64 || cfg->width > 64;
    out.tile_h = th;
    out.tile_w = tw;
    out.segs.clear();
    if (cfg->n_layers < 1) return fail(NF_EINVAL, "n_layers must be >= 1");
    if (cfg->flags & ~(NF_CFG_FP16_CNN | NF_CFG_EXACT_FP32 | NF_CFG_GRAD_MFMA | NF_CFG_GRAD_TILED | NF_CFG_GRAD_TILED_WIDE | NF_CFG_GRAD_GEMM | NF_CFG_GRAD_TILED_GEMM | NF_CFG_SVJP_MFMA | NF_CFG_SVJP_TILED | NF_CFG_SVJP_GEMM)) return fail(NF_EINVAL, "nf_config.flags has unknown bits set");
    const double HW = (double)cfg->height * cfg->width;

    // intermediate list in NLL order
    struct Item {
        int type;               // NF_OP_* of the NLL direction
        std::vector<float> blk; // folded block (fwd)
        Mat4 A, Ainv;
        double scale = 1.0;     // gain value for SCALE items
        int w = 0;
        int slot = 0;           // conditioning slot of SDN / SCALE_COND items
    };
    std::vector<Item> items;
    int width = 0, raw_width = 0;   // width of the kernels' layouts / of the model's variables (differ when zero-padded)
    out.ld_const = 0.0;
    out.has_sdn = false;
    out.cond.clear();
    for (int li = 0; li < cfg->n_layers; ++li) {
        const nf_layer_desc &L = layers[li];
        const int64_t cnt = nf_param_count(L.type, L.width);
        if (cnt < 0) return fail(NF_EINVAL, "layer %d: unknown type %d / width %d", li, L.type, L.width);
        if (L.param_offset < 0 || (uint64_t)L.param_offset + (uint64_t)cnt > n_params)
            return fail(NF_EINVAL, "layer %d: parameters [%lld, +%lld) exceed n_params=%zu", li,
                        (long long)L.param_offset, (long long)cnt, n_params);
        const float *p = params + L.param_offset;
        Item it;
        switch (nf_layer_info(L.type).cls) {
        case NF_CLS_MIX: {
            double lad = 0.0;
            bool ok = true;
            if (L.type == NF_LAYER_CONV1X1) fold_conv1x1(p, it.A, it.Ainv, lad);
            else if (L.type == NF_LAYER_CONV1X1_LU2) ok = fold_conv1x1_lu2(p, it.A, it.Ainv, lad);
            else if (L.type == NF_LAYER_CONV1X1_NONE) ok = nf_invert4(it.A = nf_mat_of(p), it.Ainv, lad);
            else {
                nf_mat_reverse(&it.A.m[0][0]);
                it.Ainv = it.A;
            }
            if (!ok) return fail(NF_EINVAL, "layer %d: the 1x1 matrix is singular", li);
            it.type = NF_OP_MIX;
            out.ld_const += HW * lad;                       // layers.py:129-130
            break;
        }
        case NF_CLS_COUPLING: {
            if (L.width < 1 || L.width > 512)
                return fail(NF_EINVAL, "layer %d: coupling width %d unsupported (1 .. 512)", li, L.width);
            // layers.py:452-498 takes any width; the kernels exist for 4 / 8 / 16 / 32 and, zero-padded inside their layouts, 33 .. 512.
            // Widths in between run on the next kernel up, zero-padded HERE: a hidden channel with zero weights and zero bias is
            // relu(0) = 0 in both hidden layers and contributes nothing to l_2 / l_last — exact.
            const int wk = L.width > 32 ? L.width : L.width <= 4 ? 4 : L.width <= 8 ? 8 : L.width <= 16 ? 16 : 32;
            if (L.width > 32 && !nf_gemm_shape_ok(th, tw))
                return fail(NF_EINVAL, "layer %d: coupling width %d covers patches of up to %d pixels (%dx%d given)", li, L.width,
                            NF7_MAX_PIXELS, cfg->height, cfg->width);
            if (raw_width && raw_width != L.width) return fail(NF_EINVAL, "all coupling layers must share one width");
            raw_width = L.width;
            width = wk;
            it.type = NF_OP_COUPLING_FWD;
            it.w = wk;
            it.blk.assign(nf_cpl_size(wk), 0.0f);
            fold_coupling(p, L.width, wk, it.blk.data());
            break;
        }
        case NF_CLS_SDN:
        case NF_CLS_COND_GAIN:
            if (out.cond.size() >= 4) return fail(NF_EINVAL, "at most 4 conditional (sdn/gain) layers per model");
            it.type = is_gain_kind(L.type) ? NF_OP_SCALE_COND : NF_OP_SDN_DIV;
            it.slot = (int)out.cond.size();
            out.cond.push_back(CondLayer{L.type, std::vector<float>(p, p + cnt)});
            if (!is_gain_kind(L.type)) out.has_sdn = true;
            break;
        case NF_CLS_GAIN: {
            if (!(p[0] > 0.0f)) return fail(NF_EINVAL, "layer %d: gain_val must be > 0", li);
            double K;
            nf_gain_eval(L.type, p, CondIdx{}, (int)HW, it.scale, K);
            it.type = NF_OP_SCALE;
            out.ld_const -= K * log(it.scale);             // AffineCouplingGainEx4.py:114-127
            break;
        }
        case NF_CLS_NONE: break;                            // (refused above)
        }
        items.push_back(it);
    }

    // Fold every gain into a neighbouring 1x1 matrix (NLL: z/g then z@A == z@(A/g)).
    for (size_t i = 0; i < items.size(); ++i) {
        if (items[i].type != NF_OP_SCALE) continue;
        Item *tgt = nullptr;
        if (i + 1 < items.size() && items[i + 1].type == NF_OP_MIX) tgt = &items[i + 1];
        else if (i > 0 && items[i - 1].type == NF_OP_MIX) tgt = &items[i - 1];
        if (!tgt) continue;
        const double g = items[i].scale;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                tgt->A.m[r][c] /= g;
                tgt->Ainv.m[r][c] *= g;
            }
        items[i].type = 0;   // removed
    }

    std::vector<Item *> order;
    for (auto &it : items)
        if (it.type != 0) order.push_back(&it);
    if (direction == 1) std::vector<Item *>(order.rbegin(), order.rend()).swap(order);
    if (order.size() > NF_MAX_OPS) return fail(NF_EINVAL, "too many layers (%zu > %d)", order.size(), NF_MAX_OPS);

    for (Layout &l : out.lay) l = Layout();
    out.n_lds9 = 0;
    out.fp16_big = out.gemm_b = out.gemm16_b = false;
    Layout &gen = out.lay[NF_PATH_SCALAR];
    gen.prog.width = width ? width : 4;
    out.raw_width = raw_width ? raw_width : 4;
    for (Item *it : order) {
        NfOp &op = gen.prog.ops[gen.prog.n_ops++];
        op.off = (int32_t)gen.block.size();
        switch (it->type) {
        case NF_OP_MIX: {
            op.type = NF_OP_MIX;
            const Mat4 &M = direction == 0 ? it->A : it->Ainv;
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) gen.block.push_back((float)M.m[r][c]);
            break;
        }
        case NF_OP_COUPLING_FWD:
            op.type = direction == 0 ? NF_OP_COUPLING_FWD : NF_OP_COUPLING_REV;
            gen.block.insert(gen.block.end(), it->blk.begin(), it->blk.end());
            break;
        case NF_OP_SDN_DIV:
            op.type = direction == 0 ? NF_OP_SDN_DIV : NF_OP_SDN_MUL;
            op.off = it->slot;
            break;
        case NF_OP_SCALE_COND:
            op.type = NF_OP_SCALE_COND;
            op.off = it->slot;
            break;
        case NF_OP_SCALE: {
            op.type = NF_OP_SCALE;
            const double s = direction == 0 ? 1.0 / it->scale : it->scale;
            gen.block.push_back((float)s);
            gen.block.push_back(0.f);
            gen.block.push_back(0.f);
            gen.block.push_back(0.f);
            break;
        }
        }
    }
    if (gen.block.empty()) gen.block.assign(4, 0.0f);

    // Every other family, where the model qualifies: the condition under which its layout exists, then build_layout
    const int w = gen.prog.width;
    const bool fp16_cnn = (cfg->flags & NF_CFG_FP16_CNN) != 0;
    // matrix-core re-layout (j-major weights)
    Layout &mfma4 = out.lay[NF_PATH_MFMA4];
    if (w == 4) {
        build_layout(gen, mfma4, 4, true, NF2_CPL_SIZE, relayout_coupling_v2);
        if (mfma4.block.size() > NF2_MAX_FLOATS) mfma4.block.clear();   // too large for LDS: scalar path only
    }
    // split-bf16 layout: the default kernel of the fp32 width-4 model on full 32x32 patches
    if (w == 4 && !mfma4.block.empty() && cfg->height == 32 && cfg->width == 32 && !(cfg->flags & (NF_CFG_FP16_CNN | NF_CFG_EXACT_FP32))) {
        Layout &split = out.lay[NF_PATH_SPLIT_BF16];
        std::vector<uint32_t> img;
        std::vector<int> aoff_at;   // LDS-part offsets of the couplings' AOFF fields
        build_layout(gen, split, 4, true, NF12_CPL_SIZE, [&](const float *v1, float *o) {
            img.resize(img.size() + NF12_A_SIZE);
            relayout_coupling_v12(v1, o, img.data() + img.size() - NF12_A_SIZE);
            aoff_at.push_back((int)(o - split.block.data()) + NF12_CPL_AOFF);
        });
        out.n_lds9 = (int)split.block.size();   // a multiple of 4: every section is
        for (size_t c = 0; c < aoff_at.size(); ++c) {
            const int32_t off = out.n_lds9 + (int32_t)(c * NF12_A_SIZE);
            memcpy(split.block.data() + aoff_at[c], &off, 4);
        }
        const size_t n0 = split.block.size();
        split.block.resize(n0 + img.size());
        if (!img.empty()) memcpy(split.block.data() + n0, img.data(), img.size() * 4);
        // Not reachable today: this layout exists only where the NF_PATH_MFMA4 block fits NF2_MAX_FLOATS (above), an op costs here at most what it
        // costs there, and a coupling 96 floats against 332 — with c couplings, m mixes (m <= c) and s scales in NF_MAX_OPS = 64
        // ops, 332 c + 16 m + 4 s <= 6144 gives c <= 17 (18 without mixes) and 96 c + 16 m + 4 s <= 2024 (tests/test_split_bf16.py
        // finds the boundary through nf_fold_layout for flow_permutation 0 / 1 / 2).  Kept as the guard of the kernel's LDS budget
        // should either limit or a section size change.
        if (out.n_lds9 > NF12_MAX_FLOATS) {   // LDS image too large for 4 workgroups per CU: the exact-fp32 kernel
            split.block.clear();
            out.n_lds9 = 0;
        }
    }
    // width 32: the product path; width 8 only where the scalar-weight kernel's LDS tile does not fit (patches larger
    // than 48x48): zero-padded to 32 channels.  Width 16 has its own kernel (NF_PATH_WIDE16).
    // tiled images (nf_device.h): width 8 runs zero-padded on the width-32 kernel; width 16 on its own (fp32; its fp16-CNN
    // mode is the width-32 fp16 kernel's, tiled or not)
    const size_t tile_px = ((size_t)(th + 2) * (tw + 2) + 1) & ~(size_t)1;
    const bool scalar_fits = sizeof(float) * (tile_px * (2 + (size_t)w) + 64) <= 160 * 1024;
    if (w == 32 || (w == 8 && !scalar_fits) || (out.tiled && w == 8))
        build_layout(gen, out.lay[NF_PATH_WIDE32], 32, false, NF4_CPL_SIZE, [&](const float *v1, float *o) { relayout_coupling_wide32(v1, w, o); });
    if (w == 16)
        build_layout(gen, out.lay[NF_PATH_WIDE16], 16, false, NF6_CPL_SIZE, [&](const float *v1, float *o) { relayout_coupling_wide16(v1, w, o); });
    if (w > 32 && fp16_cnn) {
        const int wp = nf7_pad_width(w);
        // variant B (weights resident in LDS, pixel tiles per wavefront) where its slabs fit: widths <= 128; NF_GEMM16=a: A/B aid
        const char *e = getenv("NF_GEMM16");
        const bool vb = out.gemm16_b = nf_gemm16b_shape_ok(wp, th, tw) && !(e && e[0] == 'a');
        build_layout(gen, out.lay[NF_PATH_GEMM_FP16], wp, false, vb ? nf9_cpl_size(wp) : nf8_cpl_size(wp),
                     [&](const float *v1, float *o) { vb ? relayout_coupling_gemm16b(v1, w, wp, o) : relayout_coupling_gemm16(v1, w, wp, o); });
    }
    if (w > 32 && !fp16_cnn) {
        const int wp = nf7_pad_width(w);
        // variant B where its slabs fit beside the patch's tiles; NF_GEMM=a: A/B aid
        const char *e = getenv("NF_GEMM");
        const bool vb = out.gemm_b = nf_gemmb_shape_ok(wp, th, tw) && !(e && e[0] == 'a');
        build_layout(gen, out.lay[NF_PATH_GEMM], wp, false, vb ? nf10_cpl_size(wp) : nf7_cpl_size(wp),
                     [&](const float *v1, float *o) { vb ? relayout_coupling_gemmb(v1, w, wp, o) : relayout_coupling_gemm(v1, w, wp, o); });
    }
    // width 4 has its own fp16 kernel for the two full shapes (nf_kernels.hip); on any other shape it runs here, zero-padded
    // to 32 channels (exact: same rounding points, a padded channel is identically zero)
    // NF_H16=4x4 (read at nf_create) keeps the v_mfma_f32_4x4x4_16b_f16 formulation of the width-4 fp16 kernel — an A/B aid
    const bool fp16_big = [] { const char *e = getenv("NF_H16"); return !(e && strcmp(e, "4x4") == 0); }();
    // width 4 in fp16-CNN mode has its own kernel for full 32x32 / 64x64 patches — and, on v_mfma_f32_16x16x32_f16, for images
    // tiled into full 64x64 tiles; everything else rides the width-32 fp16 kernel zero-padded
    const bool w4_full = ((th == 32 && tw == 32) || (th == 64 && tw == 64)) && (!out.tiled || (fp16_big && th == 64 && tw == 64));
    if (fp16_cnn && (w == 8 || w == 16 || w == 32 || (w == 4 && !w4_full)))
        build_layout(gen, out.lay[NF_PATH_WIDE32_FP16], 32, false, NF5_CPL_SIZE, [&](const float *v1, float *o) { relayout_coupling_wide32_fp16(v1, w, o); });
    if (w == 4 && fp16_cnn) {
        out.fp16_big = fp16_big;
        // 64x64 patches / tiles: l_2's operands for v_mfma_f32_16x16x32_f16 ride along (NF11_CPL_A2)
        const bool with_a2 = th == 64 && tw == 64;
        Layout &fp16 = out.lay[NF_PATH_FP16];
        build_layout(gen, fp16, 4, true, fp16_big ? (with_a2 ? NF11_CPL_SIZE_L2 : NF11_CPL_SIZE) : NF3_CPL_SIZE,
                     [&](const float *v1, float *o) { fp16_big ? relayout_coupling_v11(v1, o, with_a2) : relayout_coupling_v3(v1, o); });
        if (fp16.block.size() > (size_t)(fp16_big ? NF11_MAX_FLOATS : NF2_MAX_FLOATS)) return fail(NF_EINVAL, "model too large for the fp16-CNN LDS image");
    }
    if (out.tiled) {
        // every coupling widens the dependence of a pixel by 2 (3x3, 1x1, 3x3): nf_device.h, "overlapping tiles"
        int rc = plan_tile_segments(gen.prog, cfg->height, cfg->width, th, tw, out.segs);
        if (rc != NF_OK) return rc;
    }
    return NF_OK;
}

// ---- input gradients (nf_nll_grad, nf_grad.hip, nf_grad_wide.hip) -----------------------------------
// NF_GRAD=scalar sends a handle with NF_CFG_GRAD_MFMA to the scalar-weight gradient kernel wherever that kernel holds the shape (A/B aid)
bool grad_force_scalar()
{
    static const bool fs = [] {
        const char *e = getenv("NF_GRAD");
        return e && strcmp(e, "scalar") == 0;
    }();
    return fs;
}

// THE place that decides what nf_nll_grad supports and which kernel runs it (`path`: NF_GRAD_PATH_*): `fwd` = the NLL-direction
// program of the model.
// `tiles` (NF_GRAD_PATH_TILED, NF_GRAD_PATH_TILED_WIDE32 and NF_GRAD_PATH_TILED_GEMM only): the segments of the tiled route, gradient halos and the backward
// launches' tile counts.
int grad_support(const nf_config *cfg, const Built &fwd, int *path = nullptr, std::vector<Built::TileSeg> *tiles = nullptr)
{
    if (path) *path = NF_GRAD_PATH_SCALAR;
    if (tiles) tiles->clear();
    // NF_CFG_GRAD_GEMM: coupling widths beyond 32 — and nothing else — on the GEMM gradient kernel (nf_grad_gemm.hip): whole patches of
    // up to 32x32, fp32 handles, no tile mode whatever the other tile flags say.  NF_CFG_GRAD_TILED_GEMM: all of that, and every other
    // shape on 32-pixel tiles of the same kernel, one launch per segment (kGradGemmSegs).  NF_CFG_SVJP_GEMM includes NF_CFG_GRAD_GEMM:
    // one gradient block serves nf_nll_grad and nf_sample_vjp
    if ((cfg->flags & (NF_CFG_GRAD_GEMM | NF_CFG_GRAD_TILED_GEMM | NF_CFG_SVJP_GEMM)) && fwd.lay[NF_PATH_SCALAR].prog.width > 32) {
        const NfProgram &gprog = fwd.lay[NF_PATH_SCALAR].prog;
        const bool gemm_tiles = (cfg->flags & NF_CFG_GRAD_TILED_GEMM) != 0;
        if (cfg->flags & NF_CFG_FP16_CNN)
            return fail(NF_EINVAL, "nf_nll_grad: coupling width %d under NF_CFG_GRAD_GEMM takes fp32 handles only (NF_CFG_FP16_CNN is set)", fwd.raw_width);
        if ((cfg->height > 32 || cfg->width > 32) && !gemm_tiles)
            return fail(NF_EINVAL, "nf_nll_grad: coupling width %d under NF_CFG_GRAD_GEMM covers whole patches of up to 32x32 (%dx%d given; no tile mode at "
                                   "widths beyond 32, with or without NF_CFG_GRAD_TILED / NF_CFG_GRAD_TILED_WIDE)", fwd.raw_width, cfg->height, cfg->width);
        int n_gc = 0;
        for (int i = 0; i < gprog.n_ops; ++i) n_gc += gprog.ops[i].type == NF_OP_COUPLING_FWD ? 1 : 0;
        if (n_gc > NFGG_MAX_COUPLINGS)
            return fail(NF_EINVAL, "nf_nll_grad: at most %d couplings at coupling width %d under NF_CFG_GRAD_GEMM (%d given): the gate record in device "
                                   "scratch", NFGG_MAX_COUPLINGS, fwd.raw_width, n_gc);
        if (cfg->height > 32 || cfg->width > 32) {
            std::vector<Built::TileSeg> segs;
            const int th = cfg->height < NF_GRAD_TILE ? cfg->height : NF_GRAD_TILE, tw = cfg->width < NF_GRAD_TILE ? cfg->width : NF_GRAD_TILE;
            const int rc = plan_tile_segments(gprog, cfg->height, cfg->width, th, tw, segs, kGradGemmSegs);
            if (rc != NF_OK) return rc;
            if (path) *path = NF_GRAD_PATH_TILED_GEMM;
            if (tiles) tiles->swap(segs);
            return NF_OK;
        }
        if (path) *path = NF_GRAD_PATH_GEMM;
        return NF_OK;
    }
    if (cfg->flags & NF_CFG_FP16_CNN) return fail(NF_EINVAL, "nf_nll_grad: fp32 handles only (NF_CFG_FP16_CNN is set)");
    const bool whole = cfg->height <= 64 && cfg->width <= 64;   // one workgroup's patch
    // NF_CFG_SVJP_TILED includes NF_CFG_GRAD_TILED: one gradient block and one plan serve nf_nll_grad and nf_sample_vjp
    const bool tile_flag = (cfg->flags & (NF_CFG_GRAD_TILED | NF_CFG_SVJP_TILED)) != 0;
    const bool wide_flag = (cfg->flags & NF_CFG_GRAD_TILED_WIDE) != 0;
    if (!whole && !tile_flag && !wide_flag)
        return fail(NF_EINVAL, "nf_nll_grad: patches of up to 64x64 (%dx%d given; no tiled evaluation)", cfg->height, cfg->width);
    const NfProgram &prog = fwd.lay[NF_PATH_SCALAR].prog;
    const int w = prog.width, hw = cfg->height * cfg->width;
    if (w > 32) return fail(NF_EINVAL, "nf_nll_grad: coupling widths up to 32 (%d given; the GEMM families have no gradient kernel)", fwd.raw_width);
    // NF_CFG_GRAD_TILED_WIDE: at padded width 32 — and nowhere else — everything NF_CFG_GRAD_MFMA does plus tiles of its kernel
    const bool wide_tiles = wide_flag && w == 32;
    if (!whole && !tile_flag && !wide_tiles)
        return fail(NF_EINVAL, "nf_nll_grad: patches of up to 64x64 (%dx%d given; no tiled evaluation)", cfg->height, cfg->width);
    int n_cpl = 0;
    for (int i = 0; i < prog.n_ops; ++i) n_cpl += prog.ops[i].type == NF_OP_COUPLING_FWD ? 1 : 0;
    const size_t lds = sizeof(float) * nf_grad_lds_floats(cfg->height, cfg->width, w, n_cpl);
    const bool scalar_holds = whole && !(hw > 1024 && w > 8) && lds <= 160 * 1024;
    if (!whole && w == 32 && !wide_tiles)
        return fail(NF_EINVAL, "nf_nll_grad: coupling width %d has no tile mode (NF_CFG_GRAD_TILED covers padded widths 4, 8 and 16): patches of up "
                               "to 64x64 as far as its whole-patch kernels hold them (%dx%d given)", fwd.raw_width, cfg->height, cfg->width);
    // Widths up to 16 under NF_CFG_GRAD_TILED — the flag only adds: a shape the whole-patch kernel does not hold goes to the same
    // kernel on 32-pixel tiles, one launch per segment (nf_device.h, "gradient tiles").  Width 32 under NF_CFG_GRAD_TILED_WIDE: a
    // shape of up to 32x32 whose gate record fits is held whole, exactly as under NF_CFG_GRAD_MFMA (below, NF_GRAD=scalar included);
    // every other shape goes to the matrix-core kernel on the same tiles — never to the scalar kernel, the slower one at this width
    const bool narrow_tiled = tile_flag && w <= 16 && !scalar_holds;
    const bool wide_tiled = wide_tiles && !(cfg->height <= 32 && cfg->width <= 32 && n_cpl <= nfgw_max_couplings(cfg->height));
    if (narrow_tiled || wide_tiled) {
        std::vector<Built::TileSeg> segs;
        const int th = cfg->height < NF_GRAD_TILE ? cfg->height : NF_GRAD_TILE, tw = cfg->width < NF_GRAD_TILE ? cfg->width : NF_GRAD_TILE;
        const int rc = plan_tile_segments(prog, cfg->height, cfg->width, th, tw, segs, wide_tiled ? kGradWideSegs : kGradSegs);
        if (rc != NF_OK) return rc;
        if (path) *path = wide_tiled ? NF_GRAD_PATH_TILED_WIDE32 : NF_GRAD_PATH_TILED;
        if (tiles) tiles->swap(segs);
        return NF_OK;
    }
    // NF_CFG_SVJP_MFMA includes NF_CFG_GRAD_MFMA: one gradient block serves nf_nll_grad and nf_sample_vjp
    if (((cfg->flags & (NF_CFG_GRAD_MFMA | NF_CFG_SVJP_MFMA)) || wide_tiles) && w == 32) {
        // The flag only adds: the matrix-core kernel (nf_grad_wide.hip) takes every shape up to 32x32 — unless NF_GRAD=scalar asks for
        // the other arm where that one holds the shape — and a shape beyond it (16x48, 8x64) stays with the scalar kernel as far as
        // that kernel holds it
        const bool wide_shape = cfg->height <= 32 && cfg->width <= 32;
        if (scalar_holds && (!wide_shape || grad_force_scalar())) return NF_OK;
        if (!wide_shape)
            return fail(NF_EINVAL, "nf_nll_grad: coupling width %d covers patches of up to 32x32 on the matrix-core gradient kernel, and the "
                                   "scalar kernel does not hold a %dx%d patch of it either (registers beyond 1024 pixels, LDS)",
                        fwd.raw_width, cfg->height, cfg->width);
        if (n_cpl > nfgw_max_couplings(cfg->height))
            return fail(NF_EINVAL, "nf_nll_grad: at most %d couplings at coupling width %d on a %dx%d patch (%d given): the gate record must fit 160 KiB of LDS",
                        nfgw_max_couplings(cfg->height), fwd.raw_width, cfg->height, cfg->width, n_cpl);
        if (path) *path = NF_GRAD_PATH_WIDE32;
        return NF_OK;
    }
    // registers: beyond 32x32 a lane of the 1 024-thread workgroup holds 4 pixels inside 128 VGPRs.  No width fits that without
    // scratch (width 4 spills 167 VGPRs, width 8 269: both run, slower); widths 16 and 32 would keep most of their hidden
    // vectors in scratch and are refused.  Width 32 keeps one pixel per lane (12 spilled VGPRs at 1 024 threads)
    if (hw > 1024 && w > 8)
        return fail(NF_EINVAL, "nf_nll_grad: coupling width %d covers patches of up to 1024 pixels (%dx%d given): registers", fwd.raw_width,
                    cfg->height, cfg->width);
    if (lds > 160 * 1024)
        return fail(NF_EINVAL, "nf_nll_grad: a %dx%d patch with coupling width %d and %d couplings needs %zu KiB of LDS (> 160)", cfg->height,
                    cfg->width, w, n_cpl, (lds + 1023) / 1024);
    return NF_OK;
}

// What nf_sample_vjp supports and which kernel runs it (`svjp_path`: NF_SVJP_PATH_*).  nf_sample_grad.hip interprets the SCALAR
// gradient block on whole patches: whatever grad_support sends to NF_GRAD_PATH_SCALAR for this model, shape and flags.  With
// NF_CFG_SVJP_MFMA, nf_sample_grad_wide.hip interprets the matrix-core block: whatever grad_support sends to NF_GRAD_PATH_WIDE32
// (that kernel keeps inside nfgw_lds_floats).  With NF_CFG_SVJP_TILED, whatever grad_support sends to NF_GRAD_PATH_TILED (padded widths
// 4 / 8 / 16) runs nf_sample_grad_kernel<.., TILED> on the gradient plan's tiles and segments (sample_vjp_tiled).  With
// NF_CFG_SVJP_GEMM, nf_sample_grad_gemm.hip interprets the GEMM block: whatever grad_support sends to NF_GRAD_PATH_GEMM (widths
// 33 .. 512, whole patches up to 32x32, at most NFGG_MAX_COUPLINGS couplings); it has no tile mode.  Either way the width, register
// and LDS limits are nf_nll_grad's: no arithmetic here.
static int sample_vjp_support_(const nf_config *cfg, const Built &fwd, int *svjp_path)
{
    if (svjp_path) *svjp_path = NF_SVJP_PATH_SCALAR;
    int path = NF_GRAD_PATH_SCALAR;
    const int rc = grad_support(cfg, fwd, &path);
    if (rc != NF_OK) {   // the limit grad_support named, under this call's name
        std::string why = g_last_error;
        const size_t at = why.find("nf_nll_grad");
        if (at != std::string::npos) why.replace(at, strlen("nf_nll_grad"), "nf_sample_vjp");
        return fail(rc, "%s", why.c_str());
    }
    if (path == NF_GRAD_PATH_TILED && (cfg->flags & NF_CFG_SVJP_TILED)) {
        if (svjp_path) *svjp_path = NF_SVJP_PATH_TILED;
        return NF_OK;
    }
    if (path == NF_GRAD_PATH_SCALAR) {
        if (fwd.lay[NF_PATH_SCALAR].prog.width == 8 && cfg->height * cfg->width > NF_SVJP_W8_MAX_PIXELS)
            return fail(NF_EINVAL, "nf_sample_vjp: coupling width %d covers patches of up to %d pixels (%dx%d given): registers", fwd.raw_width,
                        NF_SVJP_W8_MAX_PIXELS, cfg->height, cfg->width);
        return NF_OK;
    }
    if (path == NF_GRAD_PATH_WIDE32 && (cfg->flags & NF_CFG_SVJP_MFMA)) {
        if (svjp_path) *svjp_path = NF_SVJP_PATH_WIDE32;
        return NF_OK;
    }
    if (path == NF_GRAD_PATH_GEMM && (cfg->flags & NF_CFG_SVJP_GEMM)) {
        if (svjp_path) *svjp_path = NF_SVJP_PATH_GEMM;
        return NF_OK;
    }
    if (path == NF_GRAD_PATH_TILED_GEMM && (cfg->flags & NF_CFG_SVJP_GEMM))
        return fail(NF_EINVAL, "nf_sample_vjp: coupling width %d under NF_CFG_SVJP_GEMM covers whole patches of up to 32x32 (a %dx%d patch is cut "
                               "into tiles under NF_CFG_GRAD_TILED_GEMM; no tile mode yet)", fwd.raw_width, cfg->height, cfg->width);
    if (path == NF_GRAD_PATH_TILED)
        return fail(NF_EINVAL, "nf_sample_vjp: shapes the scalar gradient kernel holds whole (a %dx%d patch at coupling width %d is cut into "
                               "tiles under NF_CFG_GRAD_TILED; no tile mode yet)", cfg->height, cfg->width, fwd.raw_width);
    if (path == NF_GRAD_PATH_TILED_WIDE32 && (cfg->flags & NF_CFG_SVJP_MFMA))
        return fail(NF_EINVAL, "nf_sample_vjp: shapes the matrix-core gradient kernel holds whole (a %dx%d patch at coupling width %d is cut "
                               "into tiles under NF_CFG_GRAD_TILED_WIDE; no tile mode yet)", cfg->height, cfg->width, fwd.raw_width);
    const bool gemm = path == NF_GRAD_PATH_GEMM || path == NF_GRAD_PATH_TILED_GEMM;
    return fail(NF_EINVAL, "nf_sample_vjp: the handle's gradient block is in the %s layout (%s at coupling width %d); the scalar layout only: "
                           "no matrix-core or GEMM variant yet%s", gemm ? "GEMM" : "matrix-core",
                gemm ? "NF_CFG_GRAD_GEMM / NF_CFG_GRAD_TILED_GEMM" : "NF_CFG_GRAD_MFMA / NF_CFG_GRAD_TILED_WIDE", fwd.raw_width,
                path == NF_GRAD_PATH_WIDE32 ? " (set NF_CFG_SVJP_MFMA for the matrix-core kernel)" : "");
}

int sample_vjp_support(const nf_config *cfg, const Built &fwd, int *svjp_path = nullptr)
{
    const int rc = sample_vjp_support_(cfg, fwd, svjp_path);
    // a refusal at a width the tile mode does not cover says so beside its present words
    if (rc != NF_OK && (cfg->flags & NF_CFG_SVJP_TILED) && !(cfg->flags & NF_CFG_FP16_CNN) && fwd.lay[NF_PATH_SCALAR].prog.width > 16) {
        const std::string why = g_last_error;
        return fail(rc, "%s (NF_CFG_SVJP_TILED: tiles at coupling widths up to 16)", why.c_str());
    }
    return rc;
}

// the paths whose couplings are in the NFGW_* layout (the matrix-core kernel, whole patches or tiles); those in the NFGG_* layout
// (the GEMM kernel, likewise); the tiled paths
static bool grad_path_is_wide(int path) { return path == NF_GRAD_PATH_WIDE32 || path == NF_GRAD_PATH_TILED_WIDE32; }
static bool grad_path_is_gemm(int path) { return path == NF_GRAD_PATH_GEMM || path == NF_GRAD_PATH_TILED_GEMM; }
static bool grad_path_is_tiled(int path) { return path == NF_GRAD_PATH_TILED || path == NF_GRAD_PATH_TILED_WIDE32 || path == NF_GRAD_PATH_TILED_GEMM; }

// a.gate_words of a launch on `path`: the words of LDS gate record per pixel slot (scalar kernel) or per lane (matrix-core kernel) for
// n_cpl couplings on patches / tiles of height H; the GEMM kernel keeps its record in device scratch
static int grad_gate_words(int path, int H, int n_cpl, int width)
{
    return grad_path_is_gemm(path) ? 0 : grad_path_is_wide(path) ? nfgw_tpw(H) * n_cpl : nf_grad_gate_words(n_cpl, width);
}

static size_t round_up_256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// One coupling of the wide gradient block (nf_device.h, NFGW_*) from its generic block at width 32: the NF4_IMG_* image of the
// forward chain without the 2 log2(e) factor, and the fetch-order images of the three transposed products.
void relayout_coupling_grad_wide(const float *v1, float *out)
{
    const int w = 32;
    memcpy(out + NFGW_CPL_E, v1 + nf_cpl_off_E(w), 64 * sizeof(float));
    out[NFGW_CPL_S] = v1[nf_cpl_off_S(w)];
    out[NFGW_CPL_S + 1] = out[NFGW_CPL_S + 2] = out[NFGW_CPL_S + 3] = 0.0f;
    const float *W1 = v1 + nf_cpl_off_W1(w), *B1 = v1 + nf_cpl_off_B1(w), *W2 = v1 + nf_cpl_off_W2(w);
    const float *B2 = v1 + nf_cpl_off_B2(w), *W3 = v1 + nf_cpl_off_W3(w);
    // taps (di,dj) of the 8 off-centre row groups of a shift-add product P, by (a, g') (as relayout_coupling_wide32)
    static const int tap_of[4][2] = {{0 * 3 + 0, 2 * 3 + 0}, {0 * 3 + 2, 2 * 3 + 2}, {0 * 3 + 1, 2 * 3 + 1}, {1 * 3 + 0, 1 * 3 + 2}};
    float *img = out + NFGW_CPL_FWD;
    for (int step = 0; step < 12; ++step)
        for (int l = 0; l < 64; ++l)
            img[NF4_IMG_A1 + ((step >> 2) * 64 + l) * 4 + (step & 3)] = step < 9 ? W1[(step * 2 + (l >> 5)) * w + (l & 31)] : 0.0f;
    bias_tables32(B1, B2, 0, w, img + NF4_IMG_B1, img + NF4_IMG_B2);
    float *bwd = out + NFGW_CPL_BWD;
    for (int s = 0; s < 20; ++s)   // l_last^T: K step s = (tap s >> 1, elements j = 2 (s & 1) + K slice)
        for (int l = 0; l < 64; ++l)
            bwd[NFGW_BWD_A3T + ((s >> 2) * 64 + l) * 4 + (s & 3)] = s < 18 ? W3[((s >> 1) * w + (l & 31)) * 4 + 2 * (s & 1) + (l >> 5)] : 0.0f;
    for (int s = 0; s < 16; ++s)
        for (int l = 0; l < 64; ++l) {
            const int cin = nf4_chan(s, l >> 5), i = l & 31;
            const int a = i >> 3, gp = (i >> 2) & 1, j = i & 3;
            img[NF4_IMG_A2 + ((s >> 2) * 64 + l) * 4 + (s & 3)] = W2[cin * w + i];
            img[NF4_IMG_A3 + ((s >> 2) * 64 + l) * 4 + (s & 3)] = W3[(tap_of[a][gp] * w + cin) * 4 + j];
            bwd[NFGW_BWD_A2T + ((s >> 2) * 64 + l) * 4 + (s & 3)] = W2[i * w + cin];
            bwd[NFGW_BWD_A1T + ((s >> 2) * 64 + l) * 4 + (s & 3)] = j < 2 ? W1[((8 - tap_of[a][gp]) * 2 + j) * w + cin] : 0.0f;
        }
    for (int s = 0; s < 16; ++s)
        for (int g = 0; g < 2; ++g)
            for (int j = 0; j < 4; ++j) {
                img[NF4_IMG_A3C + ((s >> 2) * 8 + g * 4 + j) * 4 + (s & 3)] = W3[(4 * w + nf4_chan(s, g)) * 4 + j];   // centre tap (1,1)
                bwd[NFGW_BWD_A1TC + ((s >> 2) * 8 + g * 4 + j) * 4 + (s & 3)] = j < 2 ? W1[(4 * 2 + j) * w + nf4_chan(s, g)] : 0.0f;
            }
}

// One coupling of the GEMM gradient block (nf_gemm_layout.h, NFGG_*) from its generic block at width w (33 .. 512), padded to wp:
// the NF7 image of the forward chain without the 2 log2(e) factor, and the fetch-order images of the three transposed products.
void relayout_coupling_grad_gemm(const float *v1, int w, int wp, float *out)
{
    const int MT = wp / 32, KC = wp / 8;
    memcpy(out + NFGG_CPL_E, v1 + nf_cpl_off_E(w), 64 * sizeof(float));
    out[NFGG_CPL_S] = v1[nf_cpl_off_S(w)];
    out[NFGG_CPL_S + 1] = out[NFGG_CPL_S + 2] = out[NFGG_CPL_S + 3] = 0.0f;
    relayout_gemm_image(v1, w, wp, 1.0, out + NFGG_CPL_FWD);
    const float *W1 = v1 + nf_cpl_off_W1(w), *W2 = v1 + nf_cpl_off_W2(w), *W3 = v1 + nf_cpl_off_W3(w);
    float *bwd = out + nfgg_cpl_bwd(wp);
    for (int m = 0; m < MT; ++m) {
        for (int s = 0; s < 20; ++s)   // l_last^T: K step s = (tap s >> 1, elements j = 2 (s & 1) + K slice)
            for (int l = 0; l < 64; ++l) {
                const int c = 32 * m + (l & 31);
                bwd[nfgg_bwd_A3T(wp) + ((m * 5 + (s >> 2)) * 64 + l) * 4 + (s & 3)] =
                    (s < 18 && c < w) ? W3[((size_t)(s >> 1) * w + c) * 4 + 2 * (s & 1) + (l >> 5)] : 0.0f;
            }
        for (int kc = 0; kc < KC; ++kc)   // l_2^T: the output tile is an INPUT tile of W2, K runs over its output channels
            for (int l = 0; l < 64; ++l)
                for (int s2 = 0; s2 < 4; ++s2) {
                    const int kk = 4 * kc + s2, oc = 32 * (kk / 16) + nf4_chan(kk % 16, l >> 5), cin = 32 * m + (l & 31);
                    bwd[nfgg_bwd_A2T(wp) + (((size_t)m * KC + kc) * 64 + l) * 4 + s2] = (cin < w && oc < w) ? W2[(size_t)cin * w + oc] : 0.0f;
                }
        for (int v = 0; v < 16; ++v)      // l_1^T: row i = 2 tap + ch of D18, K = the channels of input tile m
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, cin = 32 * m + nf4_chan(v, l >> 5);
                bwd[nfgg_bwd_A1T(wp) + (((size_t)m * 4 + (v >> 2)) * 64 + l) * 4 + (v & 3)] = (row < 18 && cin < w) ? W1[(size_t)row * w + cin] : 0.0f;
            }
    }
}

// The gradient block (nf_device.h, NfGradLaunch): the NLL-order generic block with A^-1 beside every 1x1 matrix — op i of
// the NLL program is op n - 1 - i of the sampling program, whose block holds the inverse — and 1/s beside every scale.
// (`fwd`, `rev` = the generic layouts of the two directions).  `path` (NF_GRAD_PATH_*, grad_support) decides the couplings' layout:
// NFGW_* on the matrix-core paths at width 32 (nf_grad_wide.hip), NFGG_* at the padded width on NF_GRAD_PATH_GEMM / _TILED_GEMM (nf_grad_gemm.hip;
// the program's width is then the padded one), the generic block otherwise.
void build_grad_block(const Layout &fwd, const Layout &rev, int path, NfProgram &gp, std::vector<float> &blk, int &n_cpl, int &first_cpl)
{
    const bool wide = grad_path_is_wide(path), gemm = grad_path_is_gemm(path);
    memset(&gp, 0, sizeof(gp));
    gp.width = gemm ? nf7_pad_width(fwd.prog.width) : fwd.prog.width;
    gp.n_ops = fwd.prog.n_ops;
    blk.clear();
    n_cpl = 0;
    first_cpl = fwd.prog.n_ops;
    for (int i = 0; i < fwd.prog.n_ops; ++i) {
        const NfOp &src = fwd.prog.ops[i];
        const NfOp &inv = rev.prog.ops[fwd.prog.n_ops - 1 - i];
        const float *v = fwd.block.data() + src.off;
        gp.ops[i].type = src.type;
        gp.ops[i].off = (int32_t)blk.size();
        if (src.type == NF_OP_MIX) {
            blk.insert(blk.end(), v, v + 16);
            blk.insert(blk.end(), rev.block.data() + inv.off, rev.block.data() + inv.off + 16);
        } else if (src.type == NF_OP_COUPLING_FWD) {
            if (wide) {
                blk.resize(blk.size() + NFGW_CPL_SIZE);
                relayout_coupling_grad_wide(v, blk.data() + gp.ops[i].off);
            } else if (gemm) {
                blk.resize(blk.size() + nfgg_cpl_size(gp.width));
                relayout_coupling_grad_gemm(v, fwd.prog.width, gp.width, blk.data() + gp.ops[i].off);
            } else {
                blk.insert(blk.end(), v, v + nf_cpl_size(gp.width));
            }
            if (n_cpl == 0) first_cpl = i;
            ++n_cpl;
        } else if (src.type == NF_OP_SCALE) {
            blk.push_back(v[0]);
            blk.push_back(rev.block[inv.off]);
            blk.push_back(0.f);
            blk.push_back(0.f);
        } else {
            gp.ops[i].off = src.off;   // conditioning slot
        }
    }
    if (blk.empty()) blk.assign(4, 0.0f);
}

// a layout through the C ABI (nf_fold_params, nf_fold_layout): sizes always, contents where the caller gave room
int export_layout(const Layout &l, int32_t *ops_out, int32_t ops_cap, int32_t *n_ops, float *folded, size_t folded_cap, size_t *n_folded)
{
    if (n_ops) *n_ops = l.prog.n_ops;
    if (n_folded) *n_folded = l.block.size();
    if (ops_out) {
        if (ops_cap < l.prog.n_ops) return fail(NF_EINVAL, "ops_cap too small");
        for (int i = 0; i < l.prog.n_ops; ++i) {
            ops_out[2 * i] = l.prog.ops[i].type;
            ops_out[2 * i + 1] = l.prog.ops[i].off;
        }
    }
    if (folded) {
        if (folded_cap < l.block.size()) return fail(NF_EINVAL, "folded_cap too small");
        memcpy(folded, l.block.data(), l.block.size() * sizeof(float));
    }
    return NF_OK;
}

// NF_KERNEL=valu forces the scalar-weight VALU kernel (A/B testing); default = matrix core
bool use_matrix_core()
{
    static const bool mc = [] {
        const char *e = getenv("NF_KERNEL");
        return !(e && strcmp(e, "valu") == 0);
    }();   // read once: this sits on the per-call path
    return mc;
}

// A device buffer that grows: reserve(n) frees and reallocates only when it is too small; empty after a failed allocation.
template <class T>
struct DevBuf {
    T *ptr = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t n)
    {
        if (cap >= n) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void **)&ptr, n * sizeof(T));
        if (e != hipSuccess) ptr = nullptr;
        else cap = n;
        return e;
    }
};

}  // namespace

int nf_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fail(code, "%s", buf);
}

int nf_fail_hip(hipError_t e, const char *what) { return fail_hip(e, what); }

struct nf_bs_state;
static void nf_bs_destroy(nf_bs_state *s);

struct nf_handle {
    nf_config cfg;
    int device = 0;
    int n_cu = 256;
    Built fwd, rev;
    float *d_lay[2][NF_PATH_COUNT] = {};   // [direction][NF_PATH_*]: the layouts' blocks on the device (null: the model has none)
    bool scalar_ok = true;    // the scalar-weight kernel's LDS tiles fit this patch shape / width
    // nf_nll_grad: its program and block (nf_device.h, NfGradLaunch), or why this handle has none (grad_support)
    NfProgram gprog;
    float *d_grad = nullptr;
    int grad_n_cpl = 0, grad_first_cpl = 0;
    int grad_rc = NF_EINVAL;
    int grad_path = NF_GRAD_PATH_SCALAR;   // NF_GRAD_PATH_*: which kernel nf_nll_grad launches (grad_support)
    std::string grad_why;
    // nf_sample_vjp (nf_sample_grad.hip) runs on gprog / d_grad where sample_vjp_support says so
    int svjp_rc = NF_EINVAL;
    int svjp_path = NF_SVJP_PATH_SCALAR;   // NF_SVJP_PATH_*: which kernel nf_sample_vjp launches (sample_vjp_support)
    int svjp_last_cpl = -1;
    std::string svjp_why;
    std::vector<Built::TileSeg> grad_segs;   // NF_GRAD_PATH_TILED / _TILED_WIDE32 / _TILED_GEMM: the segments (gradient halo, tiles of the backward launches)
    int grad_seg_cpl = 0;                    // ... and the couplings of the largest one (sizes the gate record)
    // scratch of the tiled calls (images beyond 64x64): the per-tile sums and the tensors between two segments.  A small set of
    // device buffers owned by the handle, one per call in flight; a call takes a free one (waiting, on ITS stream, for the work
    // that last used it), so nf_nll / nf_sample allocate only when a call needs more than any earlier one did, or when more
    // calls are in flight than ever before — nf_reserve_workspace sizes it up front
    struct Workspace {
        char *p = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;   // recorded behind the last launch that used the buffer
        bool busy = false;         // a host thread is enqueueing on it
        bool used = false;         // `ev` was recorded behind real work (a freshly reserved buffer has no prior user to wait for)
    };
    std::mutex ws_mu;
    std::vector<Workspace *> ws;
    // batch-statistics mode (nf_*_batchstats): the raw model and a lazily allocated scratch
    std::vector<nf_layer_desc> layers;
    std::vector<float> raw;
    std::mutex bs_mu;
    struct nf_bs_state *bs = nullptr;
    // cross-rank batch statistics of nf_*_batchstats (nf_set_sync)
    nf_allreduce_fn sync_fn = nullptr;
    void *sync_user = nullptr;
    double *sync_buf = nullptr;
    int sync_world = 1;
};

int nf_handle_geometry(const nf_handle *h, int32_t *H, int32_t *W, int32_t *device)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    *H = h->cfg.height;
    *W = h->cfg.width;
    *device = h->device;
    return NF_OK;
}

extern "C" {

int nf_destroy(nf_handle *h);

int nf_abi_version(void) { return NF_ABI_VERSION; }

const char *nf_last_error(void) { return g_last_error.c_str(); }

int64_t nf_layer_param_count(int32_t type, int32_t width) { return nf_param_count(type, width); }

int nf_fold_params(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params,
                   int32_t direction, int32_t *ops_out, int32_t ops_cap, int32_t *n_ops, float *folded,
                   size_t folded_cap, size_t *n_folded, double *ld_const)
{
    if (direction != 0 && direction != 1) return fail(NF_EINVAL, "direction must be 0 or 1");
    Built b;
    int rc = build_program(cfg, layers, params, n_params, direction, b);
    if (rc != NF_OK) return rc;
    if (ld_const) *ld_const = b.ld_const;
    return export_layout(b.lay[NF_PATH_SCALAR], ops_out, ops_cap, n_ops, folded, folded_cap, n_folded);
}

int nf_fold_layout(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int32_t direction,
                   int32_t path, int32_t *ops_out, int32_t ops_cap, int32_t *n_ops, int32_t *layout_width, float *folded,
                   size_t folded_cap, size_t *n_folded)
{
    if (direction != 0 && direction != 1) return fail(NF_EINVAL, "direction must be 0 or 1");
    Built b;
    int rc = build_program(cfg, layers, params, n_params, direction, b);
    if (rc != NF_OK) return rc;
    if (path < 0 || path >= NF_PATH_COUNT) return fail(NF_EINVAL, "unknown kernel path %d", path);
    const Layout &l = b.lay[path];
    if (l.block.empty()) return fail(NF_EINVAL, "this model has no parameter block for kernel path %d", path);
    if (layout_width) *layout_width = l.prog.width;
    return export_layout(l, ops_out, ops_cap, n_ops, folded, folded_cap, n_folded);
}

int nf_split_run_info(const int32_t *ops, int32_t n_ops, const float *block, size_t n_block, int32_t out[8])
{
    if (!ops || !block || !out || n_ops < 0 || n_ops > NF_MAX_OPS) return fail(NF_EINVAL, "bad argument");
    NfProgram prog;
    memset(&prog, 0, sizeof(prog));
    prog.width = 4;
    prog.n_ops = n_ops;
    for (int i = 0; i < n_ops; ++i) {
        prog.ops[i].type = ops[2 * i];
        prog.ops[i].off = ops[2 * i + 1];
    }
    NfLaunch a;
    memset(&a, 0, sizeof(a));
    nf_find_run(prog, block, n_block, a);
    const int32_t v[8] = {a.run_first, a.run_n, a.run_moff, a.run_coff, a.run_stride, a.run_type, a.run_aoff, a.run_astride};
    memcpy(out, v, sizeof(v));
    return NF_OK;
}

int nf_sdn5_scalars(const float *sdn_params, const nf_cond *cond, double out[2])
{
    if (!sdn_params || !out) return fail(NF_EINVAL, "null argument");
    return cond_scalars(NF_LAYER_SDN5, sdn_params, cond, out);
}

int nf_create(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, nf_handle **out)
{
    if (!out) return fail(NF_EINVAL, "out is NULL");
    *out = nullptr;
    nf_handle *h = new (std::nothrow) nf_handle();
    if (!h) return fail(NF_ENOMEM, "out of host memory");
    int rc = build_program(cfg, layers, params, n_params, 0, h->fwd);
    if (rc == NF_OK) rc = build_program(cfg, layers, params, n_params, 1, h->rev);
    if (rc != NF_OK) {
        delete h;
        return rc;
    }
    h->cfg = *cfg;
    h->layers.assign(layers, layers + cfg->n_layers);
    h->raw.assign(params, params + n_params);
    {   // the two LDS tiles of the scalar-weight kernel must fit one CU (160 KiB)
        const size_t tile_px = ((size_t)(h->fwd.tile_h + 2) * (h->fwd.tile_w + 2) + 1) & ~(size_t)1;
        const int w = h->fwd.lay[NF_PATH_SCALAR].prog.width;
        const size_t lds = sizeof(float) * (tile_px * (2 + (size_t)w) + 64);
        h->scalar_ok = lds <= 160 * 1024 && w <= 32;
        bool other = false;   // a family that takes the patch instead (NF_PATH_FP16 and NF_PATH_SPLIT_BF16 are not asked)
        for (int p : {NF_PATH_MFMA4, NF_PATH_WIDE32, NF_PATH_WIDE32_FP16, NF_PATH_WIDE16, NF_PATH_GEMM, NF_PATH_GEMM_FP16})
            other = other || !h->fwd.lay[p].block.empty();
        if (lds > 160 * 1024 && !other) {
            delete h;
            return fail(NF_EINVAL, "a %dx%d patch with coupling width %d needs %zu KiB of LDS (> 160): unsupported",
                        cfg->height, cfg->width, w, lds / 1024);
        }
    }
    hipError_t e;
    if (cfg->device >= 0) {
        h->device = cfg->device;
    } else if ((e = hipGetDevice(&h->device)) != hipSuccess) {
        delete h;
        return fail_hip(e, "hipGetDevice");
    }
    NfDeviceGuard guard;
    if ((rc = guard.enter(h->device)) != NF_OK) {
        delete h;
        return rc;
    }
    int n_cu = 0;
    if ((e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, h->device)) != hipSuccess) {
        delete h;
        return fail_hip(e, "hipDeviceGetAttribute");
    }
    h->n_cu = n_cu > 0 ? n_cu : 256;
    if (cfg->flags & NF_CFG_FP16_CNN) {
        const int hw = cfg->height * cfg->width;
        const bool w4_ok = !h->fwd.lay[NF_PATH_FP16].block.empty() &&
                           ((cfg->height == 32 && cfg->width == 32) || (cfg->height == 64 && cfg->width == 64) ||
                            (h->fwd.tiled && h->fwd.fp16_big && h->fwd.tile_h == 64 && h->fwd.tile_w == 64));
        if ((!w4_ok && h->fwd.lay[NF_PATH_WIDE32_FP16].block.empty() && h->fwd.lay[NF_PATH_GEMM_FP16].block.empty()) || hw == 0) {
            nf_destroy(h);
            return fail(NF_EINVAL, "NF_CFG_FP16_CNN: no half-precision kernel for this width / patch shape");
        }
    }
    for (int p = 0; p < NF_PATH_COUNT; ++p)   // every layout the model has, both directions
        for (int d = 0; d < 2; ++d) {
            const std::vector<float> &blk = (d == 0 ? h->fwd : h->rev).lay[p].block;
            if (blk.empty()) continue;
            const bool gen = p == NF_PATH_SCALAR;
            if ((e = hipMalloc((void **)&h->d_lay[d][p], blk.size() * sizeof(float))) != hipSuccess) {
                nf_destroy(h);
                return fail_hip(e, gen ? "hipMalloc(params)" : "hipMalloc/hipMemcpy(matrix-core params)");
            }
            if ((e = hipMemcpy(h->d_lay[d][p], blk.data(), blk.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
                nf_destroy(h);
                return fail_hip(e, gen ? "hipMemcpy(params)" : "hipMalloc/hipMemcpy(matrix-core params)");
            }
        }
    {   // the gradient kernel's block, where nf_nll_grad supports the model (otherwise the call reports grad_why)
        const std::string keep = g_last_error;
        h->grad_rc = grad_support(cfg, h->fwd, &h->grad_path, &h->grad_segs);
        h->grad_why = g_last_error;
        for (const Built::TileSeg &g : h->grad_segs) h->grad_seg_cpl = std::max(h->grad_seg_cpl, g.halo / kGradSegs.halo_per_cpl);
        g_last_error = keep;
        if (h->grad_rc == NF_OK) {
            std::vector<float> gb;
            build_grad_block(h->fwd.lay[NF_PATH_SCALAR], h->rev.lay[NF_PATH_SCALAR], h->grad_path, h->gprog, gb,
                             h->grad_n_cpl, h->grad_first_cpl);
            if ((e = hipMalloc((void **)&h->d_grad, gb.size() * sizeof(float))) != hipSuccess ||
                (e = hipMemcpy(h->d_grad, gb.data(), gb.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) {
                nf_destroy(h);
                return fail_hip(e, "hipMalloc/hipMemcpy(gradient params)");
            }
        }
        const std::string keep2 = g_last_error;
        h->svjp_rc = sample_vjp_support(cfg, h->fwd, &h->svjp_path);
        h->svjp_why = g_last_error;
        g_last_error = keep2;
        for (int i = 0; h->svjp_rc == NF_OK && i < h->gprog.n_ops; ++i)
            if (h->gprog.ops[i].type == NF_OP_COUPLING_FWD) h->svjp_last_cpl = i;
    }
    *out = h;
    return NF_OK;
}

int nf_destroy(nf_handle *h)
{
    if (!h) return NF_OK;
    nf_hostpipe_release(h);
    NfDeviceGuard guard;
    (void)guard.enter(h->device);
    for (auto &dir : h->d_lay)
        for (float *p : dir)
            if (p) (void)hipFree(p);
    if (h->d_grad) (void)hipFree(h->d_grad);
    nf_bs_destroy(h->bs);
    for (nf_handle::Workspace *w : h->ws) {
        if (w->ev) {
            (void)hipEventSynchronize(w->ev);
            (void)hipEventDestroy(w->ev);
        }
        if (w->p) (void)hipFree(w->p);
        delete w;
    }
    delete h;
    return NF_OK;
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What the kernels read of one nf_cond (NfLaunch::cond_a / cond_b and the per-call part of the constant log-det, or one row of a
// per-patch call): the scalars of the program's conditional layers in slot order.  direction 0 (NLL) divides by a gain layer's
// scale and carries its log-det; direction 1 (sampling) multiplies.  Unused slots stay a = 0, b = 1.
static int cond_row_of(const Built &b, int H, int W, int direction, const nf_cond *cond, nf_cond_row &r)
{
    for (int i = 0; i < 4; ++i) {
        r.a[i] = 0.f;
        r.b[i] = 1.f;
    }
    r.ld = 0.0;   // per-call part of the constant log-det (plain `gain` layers)
    r.reserved = 0.0;
    for (size_t i = 0; i < b.cond.size(); ++i) {
        double sc[2], K = 0.0;
        int rc = cond_scalars(b.cond[i].kind, b.cond[i].p.data(), cond, sc, H * W, &K);
        if (rc != NF_OK) return rc;
        if (direction == 0 && is_gain_kind(b.cond[i].kind)) {
            r.a[i] = (float)(1.0 / sc[0]);            // NLL direction divides
            r.ld -= K * log(sc[0]);
        } else {
            r.a[i] = (float)sc[0];                    // sampling direction multiplies
            r.b[i] = (float)sc[1];
        }
    }
    return NF_OK;
}

// the rows of a per-patch call: [B] on the handle's device, 16-byte aligned
static int check_rows(const nf_handle *h, const nf_cond_row *rows, int64_t B)
{
    if (B <= 0) return NF_OK;
    if (!rows) return fail(NF_EINVAL, "rows is NULL");
    if (!aligned16(rows)) return fail(NF_EINVAL, "rows must be 16-byte aligned");
    for (const char *q : {(const char *)rows, (const char *)(rows + B) - 1}) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();
            return fail(NF_EINVAL, "rows is not device memory (all %lld rows)", (long long)B);
        }
        if (at.type != hipMemoryTypeDevice || at.device != h->device)
            return fail(NF_EINVAL, "rows must be memory of the handle's device %d", h->device);
    }
    return NF_OK;
}

// ---- argument checking + NfLaunch assembly shared by the resident and the batch-statistics paths ----
// (with_rows: a per-patch entry, whose device `rows` stand in for `cond`)
static int nll_args(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond *cond, float *nll_out,
                    float *sd_out, float *logdet_out, float *z_out, double *sums_out, uint32_t flags, NfLaunch &a,
                    bool with_rows = false, const nf_cond_row *rows = nullptr)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (B < 0) return fail(NF_EINVAL, "B must be >= 0");
    if (B > 0 && !x) return fail(NF_EINVAL, "x is NULL");
    if (h->fwd.has_sdn && B > 0 && !y) return fail(NF_EINVAL, "model has a signal-dependent layer but y is NULL");
    if (!aligned16(x) || !aligned16(y) || !aligned16(z_out))
        return fail(NF_EINVAL, "x, y and z_out must be 16-byte aligned (every pixel is one float4 access)");
    nf_cond_row r;
    if (with_rows) {   // per-patch conditioning: the kernels read rows[b], and ld_const holds the model's part only
        int rc = check_rows(h, rows, B);
        if (rc != NF_OK) return rc;
        memset(&r, 0, sizeof(r));
    } else {
        int rc = cond_row_of(h->fwd, h->cfg.height, h->cfg.width, 0, cond, r);
        if (rc != NF_OK) return rc;
    }
    memset(&a, 0, sizeof(a));
    a.in = x;
    a.y = y;
    a.out = z_out;
    a.nll_out = nll_out;
    a.sd_out = sd_out;
    a.ld_out = logdet_out;
    a.sums = sums_out;
    a.B = B;
    a.ld_const = r.ld;   // + the model's constant part, added by the launcher
    a.in_scale = 1.0f;
    memcpy(a.cond_a, r.a, sizeof(r.a));
    memcpy(a.cond_b, r.b, sizeof(r.b));
    a.cond_rows = with_rows ? rows : nullptr;
    a.H = h->cfg.height;
    a.W = h->cfg.width;
    a.flags = (flags & NF_NO_PRIOR) ? 0u : NF_K_PRIOR;
    if (flags & NF_SUMS_WIDE) a.flags |= NF_K_SUMS_WIDE;
    return NF_OK;
}

static int sample_args(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base,
                       float temp, int64_t B, const nf_cond *cond, float *x_out, NfLaunch &a, bool with_rows = false,
                       const nf_cond_row *rows = nullptr)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (B < 0) return fail(NF_EINVAL, "B must be >= 0");
    if (B > 0 && !x_out) return fail(NF_EINVAL, "x_out is NULL");
    if (h->rev.has_sdn && B > 0 && !y) return fail(NF_EINVAL, "model has a signal-dependent layer but y is NULL");
    if (!aligned16(y) || !aligned16(eps) || !aligned16(x_out))
        return fail(NF_EINVAL, "y, eps and x_out must be 16-byte aligned (every pixel is one float4 access)");
    nf_cond_row r;
    if (with_rows) {
        int rc = check_rows(h, rows, B);
        if (rc != NF_OK) return rc;
        memset(&r, 0, sizeof(r));
    } else {
        int rc = cond_row_of(h->rev, h->cfg.height, h->cfg.width, 1, cond, r);
        if (rc != NF_OK) return rc;
    }
    memset(&a, 0, sizeof(a));
    a.in = eps;
    a.y = y;
    a.out = x_out;
    a.B = B;
    a.patch_base = patch_index_base;
    a.seed = seed;
    a.in_scale = temp;
    memcpy(a.cond_a, r.a, sizeof(r.a));
    memcpy(a.cond_b, r.b, sizeof(r.b));
    a.cond_rows = with_rows ? rows : nullptr;
    a.H = h->cfg.height;
    a.W = h->cfg.width;
    a.flags = eps ? 0u : NF_K_PHILOX_IN;
    return NF_OK;
}

// ---- workspace of the tiled calls -------------------------------------------------------------------------------------
static size_t tiled_workspace_bytes(const nf_handle *h, int direction, int64_t B, bool want_sums)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    if (!b.tiled || B <= 0) return 0;
    const int S = (int)b.segs.size();
    size_t part4 = 0;
    for (int s = 0; s < S; ++s) part4 += (size_t)B * b.segs[s].ny * b.segs[s].nx;
    const size_t img = round_up_256((size_t)B * h->cfg.height * h->cfg.width * kC * sizeof(float));
    const size_t part = want_sums ? round_up_256(part4 * 4 * sizeof(float)) : 0;
    return part + img * (size_t)(S - 1 < 2 ? (S - 1 < 0 ? 0 : S - 1) : 2);
}

// a buffer of >= bytes that no other call is enqueueing on; work the stream `st` enqueues is ordered behind its last user
static int ws_acquire(nf_handle *h, size_t bytes, hipStream_t st, nf_handle::Workspace **out)
{
    *out = nullptr;
    if (bytes == 0) return NF_OK;
    nf_handle::Workspace *w = nullptr;
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lk(h->ws_mu);
        for (nf_handle::Workspace *c : h->ws)      // smallest free buffer that is large enough, else the largest free one (to grow)
            if (!c->busy && (!w || (c->bytes >= bytes ? (w->bytes < bytes || c->bytes < w->bytes) : (w->bytes < bytes && c->bytes > w->bytes)))) w = c;
        if (!w) {
            w = new (std::nothrow) nf_handle::Workspace();
            if (!w) return fail(NF_ENOMEM, "out of host memory");
            if ((e = hipEventCreateWithFlags(&w->ev, hipEventDisableTiming)) != hipSuccess) {
                delete w;
                return fail_hip(e, "hipEventCreate");
            }
            h->ws.push_back(w);
        }
        w->busy = true;                            // ours from here on: the lock is NOT held across the (device-synchronising) grow below
    }
    if (w->bytes < bytes) {                        // grow: the only allocation a call can make (the first one of its size)
        if (w->p) {
            (void)hipEventSynchronize(w->ev);
            (void)hipFree(w->p);
            w->p = nullptr;
            w->bytes = 0;
        }
        if ((e = hipMalloc((void **)&w->p, bytes)) != hipSuccess) {
            std::lock_guard<std::mutex> lk(h->ws_mu);
            w->busy = false;
            return fail_hip(e, "hipMalloc(tiled workspace)");
        }
        w->bytes = bytes;
    } else if (w->used && (e = hipStreamWaitEvent(st, w->ev, 0)) != hipSuccess) {
        std::lock_guard<std::mutex> lk(h->ws_mu);
        w->busy = false;
        return fail_hip(e, "hipStreamWaitEvent");
    }
    *out = w;
    return NF_OK;
}

static void ws_release(nf_handle *h, nf_handle::Workspace *w, hipStream_t st, bool worked = true)
{
    if (!w) return;
    if (worked) (void)hipEventRecord(w->ev, st);   // (nf_reserve_workspace only sized the buffer: nothing for its first user to wait for)
    std::lock_guard<std::mutex> lk(h->ws_mu);
    if (worked) w->used = true;
    w->busy = false;
}

// THE place that decides which kernel family a handle launches in a direction (nf_kernel_path reports it, launch_resident and
// launch_tiled dispatch on it).  A layout the model lacks has no device block.
static int select_path(const nf_handle *h, int direction)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    float *const *d = h->d_lay[direction];
    // NF_KERNEL=valu (A/B aid) selects the scalar-weight kernel only where that kernel can hold the patch
    const bool mcore = use_matrix_core() || !h->scalar_ok;
    if (d[NF_PATH_WIDE32_FP16]) return NF_PATH_WIDE32_FP16;   // NF_CFG_FP16_CNN at width 8 / 16 / 32: v_mfma_f32_32x32x16_f16
    if (d[NF_PATH_GEMM_FP16]) return NF_PATH_GEMM_FP16;       // ... at widths 33 .. 512: the GEMM kernel on the same instruction (nf_gemm16.hip)
    if (d[NF_PATH_GEMM]) return NF_PATH_GEMM;                 // widths 33 .. 512: LDS-staged GEMMs on v_mfma_f32_32x32x2_f32 (nf_gemm.hip); no other kernel holds these widths
    if (b.tiled) {   // images beyond 64x64: the GEMM and width-16 kernels take tiles as they take patches
        const int w = b.lay[NF_PATH_SCALAR].prog.width;
        if (d[NF_PATH_WIDE16] && w == 16 && mcore) return NF_PATH_WIDE16;
        if (d[NF_PATH_FP16] && b.fp16_big) return NF_PATH_FP16;   // width 4, fp16 CNN, full 64x64 tiles: the fused kernel on v_mfma_f32_16x16x32_f16
        if (d[NF_PATH_WIDE32] && w > 4) return NF_PATH_WIDE32;    // kept as found: `w > 4` and no `mcore` here, `mcore` and no width test below
        return d[NF_PATH_MFMA4] && mcore ? NF_PATH_MFMA4 : NF_PATH_SCALAR;   // kept as found: also without the matrix core when the scalar kernel cannot hold the tile
    }
    if (d[NF_PATH_WIDE16] && mcore) return NF_PATH_WIDE16;   // width 16: v_mfma_f32_16x16x4_f32 (nf_wide16.hip)
    if (d[NF_PATH_WIDE32] && mcore) return NF_PATH_WIDE32;   // width 32: the three convs on v_mfma_f32_32x32x2_f32 (nf_wide.hip)
    if (d[NF_PATH_FP16]) return NF_PATH_FP16;
    if (d[NF_PATH_SPLIT_BF16] && use_matrix_core()) return NF_PATH_SPLIT_BF16;   // width 4, fp32, full 32x32 patches: split-bf16 convs (nf_device.h, NF12_*)
    return d[NF_PATH_MFMA4] && use_matrix_core() ? NF_PATH_MFMA4 : NF_PATH_SCALAR;   // kept as found: MFMA4 only under use_matrix_core(), whatever scalar_ok says
}

// One launch of `prog` — the path's program or, tiled, a segment of it — on the path's kernel family: the path's device block,
// its size and its NF_K_* flags go into `a`.
static hipError_t launch_path(const nf_handle *h, int direction, int path, const NfProgram &prog, NfLaunch &a, hipStream_t st)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    const std::vector<float> &blk = b.lay[path].block;
    a.params = h->d_lay[direction][path];
    if (path != NF_PATH_SCALAR) a.n_params = (int32_t)blk.size();   // (the scalar-weight kernel: n_params stays what the caller set)
    switch (path) {
    case NF_PATH_WIDE32_FP16:
        a.flags |= NF_K_FP16_CNN;
        return nf_launch_wide(prog, a, h->n_cu, h->device, st);
    case NF_PATH_WIDE32: return nf_launch_wide(prog, a, h->n_cu, h->device, st);
    case NF_PATH_WIDE16: return nf_launch_wide16(prog, a, h->n_cu, h->device, st);
    case NF_PATH_GEMM_FP16:
        a.flags |= NF_K_FP16_CNN;
        return b.gemm16_b ? nf_launch_gemm16b(prog, a, h->n_cu, h->device, st) : nf_launch_gemm16(prog, a, h->n_cu, h->device, st);
    case NF_PATH_GEMM: return b.gemm_b ? nf_launch_gemmb(prog, a, h->n_cu, h->device, st) : nf_launch_gemm(prog, a, h->n_cu, h->device, st);
    case NF_PATH_SPLIT_BF16:   // the kernel holds the LDS part; the launcher reads the host block to find the couplings' A images
        a.n_params = (int32_t)b.n_lds9;
        a.flags |= NF_K_SPLIT_BF16;
        return nf_launch_flow(prog, a, h->n_cu, st, true, blk.data(), blk.size());
    case NF_PATH_FP16:
        a.flags |= NF_K_FP16_CNN | (b.fp16_big ? NF_K_FP16_BIG : 0u);
        return nf_launch_flow(prog, a, h->n_cu, st, true);
    case NF_PATH_MFMA4: return nf_launch_flow(prog, a, h->n_cu, st, true);
    default: return nf_launch_flow(prog, a, h->n_cu, st, false);
    }
}

// One tiled launch per segment of `segs` (ops [op0, op1) of the path's program, its halo and tile counts) on the direction's tiles:
// segment s reads what segment s - 1 stored (the first one a.in) and stores to outs[s] (null: nowhere); with `part`, every launch
// leaves its per-tile sums at part + tp.off[s].  a.B = images.  launch_tiled (nf_nll / nf_sample) and the forward half of a tiled
// nf_nll_grad (grad_tiled) walk their segments through here.
static hipError_t launch_segments(const nf_handle *h, int direction, const NfLaunch &a, const Built::TileSeg *segs, int n, const NfTileParts &tp,
                                  float *part, float *const *outs, hipStream_t st)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    // kernel family: fp16-CNN mode and widths 8 / 16 / 32 on the width-32 matrix-core kernel (zero-padded), width 4 in fp32 on
    // the fused width-4 kernels (select_path)
    const int path = select_path(h, direction);
    const NfProgram &full = b.lay[path].prog;
    const float *cur = a.in;
    hipError_t e = hipSuccess;
    for (int s = 0; s < n && e == hipSuccess; ++s) {
        const Built::TileSeg &g = segs[s];
        NfProgram sp;
        memset(&sp, 0, sizeof(sp));
        sp.width = full.width;
        sp.n_ops = g.op1 - g.op0;
        memcpy(sp.ops, full.ops + g.op0, sizeof(NfOp) * (size_t)sp.n_ops);
        NfLaunch t = a;
        t.B = a.B * tp.nt[s];
        t.H = b.tile_h;
        t.W = b.tile_w;
        t.img_H = h->cfg.height;
        t.img_W = h->cfg.width;
        t.tile_ny = g.ny;
        t.tile_nx = g.nx;
        t.tile_halo = g.halo;
        t.flags |= NF_K_TILED;
        if (s > 0) {   // only the first segment draws / scales the input
            t.flags &= ~(uint32_t)NF_K_PHILOX_IN;
            t.in_scale = 1.0f;
        }
        t.in = cur;
        t.out = outs[s];
        t.nll_out = t.sd_out = t.ld_out = nullptr;
        t.sums = nullptr;
        t.tile_part = part ? part + tp.off[s] * 4 : nullptr;
        e = launch_path(h, direction, path, sp, t, st);
        cur = t.out;
    }
    return e;
}

// Images beyond 64x64 (nf_device.h, "overlapping tiles"): per segment of the program one launch of the fused width-4 kernel
// (or, at widths 8 / 16 / 32 and in fp16-CNN mode, of the width-32 matrix-core kernel) over B x tiles tile-sized "patches" that reads and writes image-shaped tensors in place (the caller's, and between two
// segments a scratch tensor), then — in the NLL direction — a one-wavefront-per-image kernel that adds the tiles' sums up.  Scratch
// comes from the handle's workspace set (above): one buffer per call in flight, so concurrent calls on one handle never share it.
static int launch_tiled(nf_handle *h, int direction, NfLaunch &a, hipStream_t st, const char *what)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    const int64_t B = a.B;
    const int S = (int)b.segs.size();
    const bool want = direction == 0 && (a.nll_out || a.sd_out || a.ld_out || a.sums);
    NfTileParts tp;
    memset(&tp, 0, sizeof(tp));
    tp.n_seg = S;
    int64_t part4 = 0;   // float4 entries
    for (int s = 0; s < S; ++s) {
        tp.nt[s] = b.segs[s].ny * b.segs[s].nx;
        tp.off[s] = part4;
        if (B > (INT64_MAX / 64) / tp.nt[s]) return fail(NF_EINVAL, "B too large");
        part4 += B * tp.nt[s];
    }
    const size_t img_bytes = round_up_256((size_t)B * h->cfg.height * h->cfg.width * kC * sizeof(float));
    float *part = nullptr, *scratch[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    nf_handle::Workspace *wsp = nullptr;
    {
        const int rc = ws_acquire(h, tiled_workspace_bytes(h, direction, B, want), st, &wsp);
        if (rc != NF_OK) return rc;
        char *q = wsp ? wsp->p : nullptr;
        if (want) {
            part = reinterpret_cast<float *>(q);
            q += round_up_256((size_t)part4 * 4 * sizeof(float));
        }
        for (int i = 0; i < 2 && i < S - 1; ++i, q += img_bytes) scratch[i] = reinterpret_cast<float *>(q);
    }
    float *outs[NF_MAX_TILE_SEGS];
    for (int s = 0; s < S; ++s) outs[s] = s == S - 1 ? a.out : scratch[s & 1];
    e = launch_segments(h, direction, a, b.segs.data(), S, tp, want ? part : nullptr, outs, st);
    if (e == hipSuccess && want)
        e = nf_launch_tile_combine(part, tp, B, (double)h->cfg.height * h->cfg.width * kC, a.ld_const, a.cond_rows, a.flags, a.nll_out, a.sd_out,
                                   a.ld_out, a.sums, st);
    ws_release(h, wsp, st);
    if (e != hipSuccess) return fail_hip(e, what);
    return NF_OK;
}

// launch on the handle's resident (running-statistics) programs
static int launch_resident(nf_handle *h, int direction, NfLaunch &a, hipStream_t st, const char *what)
{
    const Built &b = direction == 0 ? h->fwd : h->rev;
    if (direction == 0) a.ld_const += b.ld_const;
    if (b.tiled) return launch_tiled(h, direction, a, st, what);
    const int path = select_path(h, direction);
    hipError_t e = launch_path(h, direction, path, b.lay[path].prog, a, st);
    if (e != hipSuccess) return fail_hip(e, what);
    return NF_OK;
}

static size_t grad_workspace_bytes(const nf_handle *h, int64_t B);

static size_t svjp_workspace_bytes(const nf_handle *h, int64_t B);

int64_t nf_workspace_bytes(const nf_handle *h, int32_t direction, int64_t B)
{
    if (!h || direction < 0 || direction > 3 || B < 0) return fail(NF_EINVAL, "bad argument");
    if (direction == 2) return (int64_t)grad_workspace_bytes(h, B);   // one tiled nf_nll_grad call
    if (direction == 3) return (int64_t)svjp_workspace_bytes(h, B);   // one tiled nf_sample_vjp call, or the gate records of NF_SVJP_PATH_GEMM
    return (int64_t)tiled_workspace_bytes(h, direction, B, direction == 0);
}

// `calls_in_flight` buffers of `need` bytes in the handle's workspace set
static int reserve_workspace(nf_handle *h, size_t need, int calls_in_flight)
{
    if (need == 0) return NF_OK;
    NfDeviceGuard guard;
    int rc = guard.enter(h->device);
    if (rc != NF_OK) return rc;
    std::vector<nf_handle::Workspace *> got;
    for (int i = 0; i < calls_in_flight && rc == NF_OK; ++i) {
        nf_handle::Workspace *w = nullptr;
        rc = ws_acquire(h, need, nullptr, &w);   // marks it busy, so that the next iteration takes (or makes) another one
        if (w) got.push_back(w);
    }
    for (nf_handle::Workspace *w : got) ws_release(h, w, nullptr, false);
    return rc;
}

int nf_reserve_workspace(nf_handle *h, int64_t B, int32_t calls_in_flight)
{
    if (!h || B < 0 || calls_in_flight < 1 || calls_in_flight > 64) return fail(NF_EINVAL, "bad argument");
    return reserve_workspace(h, std::max(tiled_workspace_bytes(h, 0, B, true), tiled_workspace_bytes(h, 1, B, false)), calls_in_flight);
}

int nf_kernel_path(const nf_handle *h, int32_t direction)
{
    if (!h || (direction != 0 && direction != 1)) return fail(NF_EINVAL, "bad argument");
    return select_path(h, direction);
}

// THE place that decides how a batch-statistics call of a handle runs (nf_batchstats_route reports it, run_batchstats switches
// on it and nothing else re-derives a part of it).  The width-4 schedule on the matrix-core kernel takes every size (images beyond
// 64x64 as overlapping tiles); the generic schedule runs on the scalar-weight kernel: both LDS tiles of a patch on one CU, one
// pixel per lane at width 32; everything else — coupling widths beyond 32, patches the scalar-weight kernel cannot hold — is a
// layer-by-layer walk on the trainer's kernels (run_batchstats_wide).  Both switches are read per call on purpose (the tests
// flip them inside one process).
static int bs_route(const nf_handle *h)
{
    const int pw = h->fwd.lay[NF_PATH_SCALAR].prog.width, H = h->cfg.height, W = h->cfg.width;
    const size_t tile_px = ((size_t)(H + 2) * (W + 2) + 1) & ~(size_t)1;
    const bool scalar_fits = sizeof(float) * (tile_px * (2 + (size_t)pw) + 64) <= 160 * 1024 && !(pw >= 32 && H * W > 1024) && h->scalar_ok && !h->fwd.tiled;
    const bool mc4 = pw == 4 && !h->fwd.lay[NF_PATH_MFMA4].block.empty() && use_matrix_core();
    const char *bw = getenv("NF_BS_WIDE");   // A/B aid: non-zero sends every call to the trainer's kernels
    // width 32 on 32x32 patches (the paper's coupling CNN on the training patch size): the evaluator runs the trainer's patch-resident
    // forward stages on the matrix cores (csrc/nf_train_pr.h) — 3 launches per coupling instead of the scalar-weight schedule
    // (1 024 patches: 3.7 -> 1.1 ms, 138: 1.24 -> 0.48).  NF_TRAIN_PR=0 keeps the scalar schedule.
    const char *pe = getenv("NF_TRAIN_PR");
    const bool pr_off = pe && atoi(pe) == 0;
    const bool pr32 = h->fwd.raw_width == 32 && H == 32 && W == 32 && !h->fwd.tiled && !pr_off;
    if (pw > 32 || pr32 || (!mc4 && !scalar_fits) || (bw && atoi(bw) != 0)) return NF_BS_ROUTE_TRAINER;
    return mc4 ? NF_BS_ROUTE_MFMA4 : NF_BS_ROUTE_SCALAR;
}

int nf_batchstats_route(const nf_handle *h)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (h->cfg.flags & NF_CFG_FP16_CNN) return fail(NF_EINVAL, "batch-statistics mode is fp32 only");
    return bs_route(h);
}

// nf_nll (one `cond` for the call) and nf_nll_percond (`with_rows`: device `rows`, one per patch)
static int nll_call(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond *cond, bool with_rows, const nf_cond_row *rows,
                    float *nll_out, float *sd_out, float *logdet_out, float *z_out, double *sums_out, uint32_t flags, void *stream,
                    const char *what)
{
    NfLaunch a;
    int rc = nll_args(h, x, y, B, cond, nll_out, sd_out, logdet_out, z_out, sums_out, flags, a, with_rows, rows);
    if (rc != NF_OK) return rc;
    NfDeviceGuard guard;
    if ((rc = guard.enter(h->device)) != NF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (sums_out && !(flags & NF_ACCUMULATE)) {
        const size_t nb = (flags & NF_SUMS_WIDE) ? (size_t)NF_SUMS_SLOTS * NF_SUMS_STRIDE : 3;
        hipError_t e = hipMemsetAsync(sums_out, 0, nb * sizeof(double), st);
        if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(sums)");
    }
    if (B == 0) return NF_OK;
    return launch_resident(h, 0, a, st, what);
}

int nf_nll(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond *cond, float *nll_out, float *sd_out,
           float *logdet_out, float *z_out, double *sums_out, uint32_t flags, void *stream)
{
    return nll_call(h, x, y, B, cond, false, nullptr, nll_out, sd_out, logdet_out, z_out, sums_out, flags, stream, "nf_nll launch");
}

// nf_sample and nf_sample_percond, as nll_call
static int sample_call(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base, float temp, int64_t B,
                       const nf_cond *cond, bool with_rows, const nf_cond_row *rows, float *x_out, void *stream, const char *what)
{
    NfLaunch a;
    int rc = sample_args(h, y, eps, seed, patch_index_base, temp, B, cond, x_out, a, with_rows, rows);
    if (rc != NF_OK) return rc;
    if (B == 0) return NF_OK;
    NfDeviceGuard guard;
    if ((rc = guard.enter(h->device)) != NF_OK) return rc;
    return launch_resident(h, 1, a, (hipStream_t)stream, what);
}

int nf_sample(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base, float temp,
              int64_t B, const nf_cond *cond, float *x_out, void *stream)
{
    return sample_call(h, y, eps, seed, patch_index_base, temp, B, cond, false, nullptr, x_out, stream, "nf_sample launch");
}

// ---- per-patch conditioning: the same launches with NfLaunch::cond_rows set ----
int nf_cond_rows(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int32_t direction,
                 const nf_cond *conds, int64_t n, nf_cond_row *rows_out)
{
    if (direction != 0 && direction != 1) return fail(NF_EINVAL, "direction must be 0 or 1");
    if (n < 0) return fail(NF_EINVAL, "n must be >= 0");
    if (n > 0 && (!conds || !rows_out)) return fail(NF_EINVAL, "conds / rows_out is NULL");
    if (!cfg) return fail(NF_EINVAL, "cfg is NULL");
    Built b;
    int rc = build_program(cfg, layers, params, n_params, direction, b);
    if (rc != NF_OK) return rc;
    for (int64_t k = 0; k < n; ++k) {
        rc = cond_row_of(b, cfg->height, cfg->width, direction, &conds[k], rows_out[k]);
        if (rc != NF_OK) {
            const std::string why = g_last_error;
            return fail(rc, "conds[%lld]: %s", (long long)k, why.c_str());
        }
    }
    return NF_OK;
}

int nf_nll_percond(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond_row *rows, float *nll_out, float *sd_out,
                   float *logdet_out, float *z_out, double *sums_out, uint32_t flags, void *stream)
{
    return nll_call(h, x, y, B, nullptr, true, rows, nll_out, sd_out, logdet_out, z_out, sums_out, flags, stream, "nf_nll_percond launch");
}

int nf_sample_percond(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base, float temp, int64_t B,
                      const nf_cond_row *rows, float *x_out, void *stream)
{
    return sample_call(h, y, eps, seed, patch_index_base, temp, B, nullptr, true, rows, x_out, stream, "nf_sample_percond launch");
}

// ---- input gradients: d nll / d x, d nll / d y (nf_grad.hip) ----
int nf_grad_supported(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params)
{
    Built b;
    int rc = build_program(cfg, layers, params, n_params, 0, b);
    if (rc != NF_OK) return rc;
    return grad_support(cfg, b);
}

int nf_grad_path(const nf_handle *h)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (h->grad_rc != NF_OK) return fail(h->grad_rc, "%s", h->grad_why.c_str());
    return h->grad_path;
}

int nf_grad_fold(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int32_t *path, int32_t *ops_out,
                 int32_t ops_cap, int32_t *n_ops, float *folded, size_t folded_cap, size_t *n_folded)
{
    Built f, r;
    int rc = build_program(cfg, layers, params, n_params, 0, f);
    if (rc == NF_OK) rc = build_program(cfg, layers, params, n_params, 1, r);
    if (rc != NF_OK) return rc;
    int gpath = NF_GRAD_PATH_SCALAR;
    if ((rc = grad_support(cfg, f, &gpath)) != NF_OK) return rc;
    Layout l;
    int n_cpl = 0, first_cpl = 0;
    build_grad_block(f.lay[NF_PATH_SCALAR], r.lay[NF_PATH_SCALAR], gpath, l.prog, l.block, n_cpl, first_cpl);
    if (path) *path = gpath;
    return export_layout(l, ops_out, ops_cap, n_ops, folded, folded_cap, n_folded);
}

// ---- nf_nll_grad on tiles (NF_CFG_GRAD_TILED, NF_CFG_GRAD_TILED_WIDE, NF_CFG_GRAD_TILED_GEMM; nf_device.h, "gradient tiles") ----
// One launch of the handle's gradient kernel: whole patches, or one segment of a tiled call (`prog` = the segment, n_cpl = the
// couplings of the call's largest segment).  scratch / bytes: the GEMM kernel's gate records.
static hipError_t grad_launch(const nf_handle *h, const NfProgram &prog, const NfGradLaunch &a, int n_cpl, void *scratch, size_t bytes, hipStream_t stream)
{
    const bool tiled = grad_path_is_tiled(h->grad_path);
    if (grad_path_is_gemm(h->grad_path)) return nf_launch_grad_gemm(prog, a, tiled, n_cpl, h->n_cu, scratch, bytes, stream);
    if (grad_path_is_wide(h->grad_path)) return nf_launch_grad_wide(prog, a, tiled, n_cpl, h->n_cu, stream);
    return nf_launch_grad(prog, a, tiled, n_cpl, h->n_cu, stream);
}

// The forward launch of segment s runs on the forward direction's own tiles (tile_h x tile_w, halo 2 per coupling)
static Built::TileSeg grad_fwd_seg(const nf_handle *h, int s)
{
    Built::TileSeg g = h->grad_segs[s];
    g.halo = g.halo / kGradSegs.halo_per_cpl * kFwdSegs.halo_per_cpl;
    g.ny = nf_tile_count(h->cfg.height, h->fwd.tile_h, g.halo);
    g.nx = nf_tile_count(h->cfg.width, h->fwd.tile_w, g.halo);
    return g;
}

static size_t grad_img_bytes(const nf_handle *h, int64_t B) { return round_up_256((size_t)B * h->cfg.height * h->cfg.width * kC * sizeof(float)); }

// NF_GRAD_PATH_TILED_GEMM: the gate records of a call, one per WORKGROUP of its largest backward launch, each sized for the couplings
// of the largest segment on one tile (nf_gemm_layout.h, nfgg_gate_halves: the function the kernel indexes by)
static size_t grad_tiled_gate_bytes(const nf_handle *h, int64_t B)
{
    if (h->grad_path != NF_GRAD_PATH_TILED_GEMM) return 0;
    int64_t most = 0;
    for (const Built::TileSeg &g : h->grad_segs) most = std::max<int64_t>(most, B * g.ny * g.nx);
    const int th = std::min(h->cfg.height, NF_GRAD_TILE), tw = std::min(h->cfg.width, NF_GRAD_TILE);
    return round_up_256((size_t)nf_grad_gemm_groups(most, h->n_cu) * nfgg_gate_halves(th * tw, h->gprog.width, h->grad_seg_cpl) * sizeof(uint16_t));
}

// scratch of one call: the forward launches' tile sums, the S - 1 tensors between two segments, two gradient tensors (ping-pong),
// NF_GRAD_PATH_TILED_GEMM: and the gate records behind them;
// NF_GRAD_PATH_GEMM: the gate records of the launch's workgroups (nf_gemm_layout.h, NFGG_*)
static size_t grad_workspace_bytes(const nf_handle *h, int64_t B)
{
    if (h->grad_rc != NF_OK || B <= 0) return 0;
    if (h->grad_path == NF_GRAD_PATH_GEMM)   // the gate records: one per WORKGROUP of the launch, not per patch
        return round_up_256((size_t)nf_grad_gemm_groups(B, h->n_cu) * nfgg_gate_halves(h->cfg.height * h->cfg.width, h->gprog.width, h->grad_n_cpl) * sizeof(uint16_t));
    if (!grad_path_is_tiled(h->grad_path)) return 0;
    const int S = (int)h->grad_segs.size();
    size_t part4 = 0;
    for (int s = 0; s < S; ++s) {
        const Built::TileSeg f = grad_fwd_seg(h, s);
        part4 += (size_t)B * f.ny * f.nx;
    }
    return round_up_256(part4 * 4 * sizeof(float)) + grad_img_bytes(h, B) * (size_t)(S - 1 + (S - 1 < 2 ? S - 1 : 2)) + grad_tiled_gate_bytes(h, B);
}

// Forward: the tiled launches of nf_nll cut at the gradient plan's boundaries, every tensor between two segments kept, and
// nf_tile_combine for nll_out.  Backward: one launch of nf_grad_kernel<.., TILED> (NF_GRAD_PATH_TILED_WIDE32: of
// nf_grad_wide_kernel<.., TILED>, over the same h->d_grad in its NFGW_* layout; NF_GRAD_PATH_TILED_GEMM: of nf_grad_gemm_kernel<.., TILED>
// over the NFGG_* layout, its gate records behind the tensors in the call's workspace buffer) per segment, last to first; segment s reads the
// tensor in front of it and the gradient segment s + 1 stored, and stores core windows — to gx_out (s = 0) or to the other of two
// scratch tensors.  gy_out: the first launch (in this order) whose segment has an SDN-kind op stores it, later ones add to it.
// Everything is enqueued on `st`.
static int grad_tiled(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond_row &r, const nf_cond_row *rows, float *nll_out,
                      float *gx_out, float *gy_out, hipStream_t st)
{
    const int S = (int)h->grad_segs.size(), H = h->cfg.height, W = h->cfg.width;
    NfTileParts tp;
    memset(&tp, 0, sizeof(tp));
    tp.n_seg = S;
    Built::TileSeg fseg[NF_MAX_TILE_SEGS];
    int64_t part4 = 0;
    for (int s = 0; s < S; ++s) {
        fseg[s] = grad_fwd_seg(h, s);
        tp.nt[s] = fseg[s].ny * fseg[s].nx;
        tp.off[s] = part4;
        const int64_t most = std::max<int64_t>(tp.nt[s], (int64_t)h->grad_segs[s].ny * h->grad_segs[s].nx);
        if (B > (INT64_MAX / 64) / most) return fail(NF_EINVAL, "B too large");
        part4 += B * tp.nt[s];
    }
    nf_handle::Workspace *wsp = nullptr;
    const int rc = ws_acquire(h, grad_workspace_bytes(h, B), st, &wsp);
    if (rc != NF_OK) return rc;
    const size_t img_bytes = grad_img_bytes(h, B);
    char *q = wsp->p;
    float *const part = reinterpret_cast<float *>(q);
    q += round_up_256((size_t)part4 * 4 * sizeof(float));
    float *inter[NF_MAX_TILE_SEGS] = {}, *gbuf[2] = {nullptr, nullptr};
    for (int s = 0; s < S - 1; ++s, q += img_bytes) inter[s] = reinterpret_cast<float *>(q);
    for (int i = 0; i < 2 && i < S - 1; ++i, q += img_bytes) gbuf[i] = reinterpret_cast<float *>(q);
    char *const gate_rec = q;   // NF_GRAD_PATH_TILED_GEMM: the gate records, the rest of the buffer
    const size_t gate_room = wsp->bytes - (size_t)(q - wsp->p);
    if (gate_room < grad_tiled_gate_bytes(h, B)) {   // refused before anything is enqueued (the launcher checks its own launch once more)
        ws_release(h, wsp, st, false);
        return fail(NF_EINVAL, "nf_nll_grad: the workspace buffer holds %zu bytes of gate records, the call needs %zu", gate_room, grad_tiled_gate_bytes(h, B));
    }

    hipError_t e = hipSuccess;
    const int n_fwd = nll_out ? S : S - 1;   // the last segment's forward launch only leaves its tile sums
    if (n_fwd > 0) {
        NfLaunch a;
        memset(&a, 0, sizeof(a));
        a.in = x;
        a.y = y;
        a.B = B;
        a.in_scale = 1.0f;
        memcpy(a.cond_a, r.a, sizeof(r.a));
        memcpy(a.cond_b, r.b, sizeof(r.b));
        a.cond_rows = rows;
        a.flags = NF_K_PRIOR;
        e = launch_segments(h, 0, a, fseg, n_fwd, tp, nll_out ? part : nullptr, inter, st);   // inter[S - 1] is null: the last one stores nothing
        if (e == hipSuccess && nll_out)
            e = nf_launch_tile_combine(part, tp, B, (double)H * W * kC, r.ld + h->fwd.ld_const, rows, NF_K_PRIOR, nll_out, nullptr, nullptr, nullptr, st);
    }
    if (e == hipSuccess && (gx_out || gy_out)) {
        NfGradLaunch a;
        memset(&a, 0, sizeof(a));
        a.params = h->d_grad;
        a.y = y;
        memcpy(a.cond_a, r.a, sizeof(r.a));
        memcpy(a.cond_b, r.b, sizeof(r.b));
        a.cond_rows = rows;
        a.H = H < NF_GRAD_TILE ? H : NF_GRAD_TILE;
        a.W = W < NF_GRAD_TILE ? W : NF_GRAD_TILE;
        a.img_H = H;
        a.img_W = W;
        a.gate_words = grad_gate_words(h->grad_path, a.H, h->grad_seg_cpl, h->gprog.width);
        bool gy_written = false;
        for (int s = S - 1; s >= 0 && e == hipSuccess; --s) {
            const Built::TileSeg &g = h->grad_segs[s];
            NfProgram sp;
            memset(&sp, 0, sizeof(sp));
            sp.width = h->gprog.width;
            sp.n_ops = g.op1 - g.op0;
            memcpy(sp.ops, h->gprog.ops + g.op0, sizeof(NfOp) * (size_t)sp.n_ops);
            NfGradLaunch t = a;
            t.first_cpl = sp.n_ops;
            bool sdn = false;
            for (int i = sp.n_ops - 1; i >= 0; --i) {
                if (sp.ops[i].type == NF_OP_COUPLING_FWD) t.first_cpl = i;
                sdn = sdn || sp.ops[i].type == NF_OP_SDN_DIV;
            }
            t.B = B * g.ny * g.nx;
            t.tile_ny = g.ny;
            t.tile_nx = g.nx;
            t.tile_halo = g.halo;
            t.z_in = s == 0 ? x : inter[s - 1];
            t.g_in = s == S - 1 ? nullptr : gbuf[(S - 2 - s) & 1];
            t.g_out = s == 0 ? gx_out : gbuf[(S - 1 - s) & 1];
            // a model without an SDN-kind op: the first segment stores the zeros
            const bool wr = gy_out && (sdn || (s == 0 && !gy_written));
            t.gy_out = wr ? gy_out : nullptr;
            t.tflags = wr && gy_written ? NF_GT_GY_ACC : 0u;
            gy_written = gy_written || wr;
            e = grad_launch(h, sp, t, h->grad_seg_cpl, gate_rec, gate_room, st);
        }
    }
    ws_release(h, wsp, st);
    if (e != hipSuccess) return fail_hip(e, "nf_nll_grad launch (tiles)");
    return NF_OK;
}

int nf_grad_tile_segments(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int32_t *out5, int32_t cap)
{
    Built b;
    int rc = build_program(cfg, layers, params, n_params, 0, b);
    if (rc != NF_OK) return rc;
    int path = NF_GRAD_PATH_SCALAR;
    std::vector<Built::TileSeg> segs;
    if ((rc = grad_support(cfg, b, &path, &segs)) != NF_OK) return rc;
    if (!grad_path_is_tiled(path)) return 0;
    for (int i = 0; i < (int)segs.size() && i < cap && out5; ++i) {
        const Built::TileSeg &g = segs[i];
        const int32_t v[5] = {g.op0, g.op1, g.halo, g.ny, g.nx};
        memcpy(out5 + 5 * i, v, sizeof(v));
    }
    return (int)segs.size();
}

int nf_reserve_grad_workspace(nf_handle *h, int64_t B, int32_t calls_in_flight)
{
    if (!h || B < 0 || calls_in_flight < 1 || calls_in_flight > 64) return fail(NF_EINVAL, "bad argument");
    return reserve_workspace(h, grad_workspace_bytes(h, B), calls_in_flight);
}

int nf_nll_grad(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond *cond, const nf_cond_row *rows, float *nll_out,
                float *gx_out, float *gy_out, void *stream)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (h->grad_rc != NF_OK) return fail(h->grad_rc, "%s", h->grad_why.c_str());
    if (B < 0) return fail(NF_EINVAL, "B must be >= 0");
    if ((cond != nullptr) == (rows != nullptr)) return fail(NF_EINVAL, "nf_nll_grad: exactly one of cond / rows must be given");
    if (B > 0 && !x) return fail(NF_EINVAL, "x is NULL");
    if (h->fwd.has_sdn && B > 0 && !y) return fail(NF_EINVAL, "model has a signal-dependent layer but y is NULL");
    if (!y && gy_out) return fail(NF_EINVAL, "gy_out must be NULL when y is");
    if (!aligned16(x) || !aligned16(y) || !aligned16(gx_out) || !aligned16(gy_out))
        return fail(NF_EINVAL, "x, y, gx_out and gy_out must be 16-byte aligned (every pixel is one float4 access)");
    nf_cond_row r;
    memset(&r, 0, sizeof(r));
    if (rows) {
        int rc = check_rows(h, rows, B);
        if (rc != NF_OK) return rc;
    } else {
        int rc = cond_row_of(h->fwd, h->cfg.height, h->cfg.width, 0, cond, r);
        if (rc != NF_OK) return rc;
    }
    if (B == 0) return NF_OK;
    if (grad_path_is_tiled(h->grad_path)) {
        NfDeviceGuard guard;
        int rc = guard.enter(h->device);
        if (rc != NF_OK) return rc;
        return grad_tiled(h, x, y, B, r, rows, nll_out, gx_out, gy_out, (hipStream_t)stream);
    }
    NfGradLaunch a;
    memset(&a, 0, sizeof(a));
    a.params = h->d_grad;
    a.x = x;
    a.y = y;
    a.nll_out = nll_out;
    a.gx_out = gx_out;
    a.gy_out = gy_out;
    a.B = B;
    a.ld_const = r.ld + h->fwd.ld_const;
    memcpy(a.cond_a, r.a, sizeof(r.a));
    memcpy(a.cond_b, r.b, sizeof(r.b));
    a.cond_rows = rows;
    a.H = h->cfg.height;
    a.W = h->cfg.width;
    a.first_cpl = h->grad_first_cpl;
    a.gate_words = grad_gate_words(h->grad_path, h->cfg.height, h->grad_n_cpl, h->gprog.width);
    NfDeviceGuard guard;
    int rc = guard.enter(h->device);
    if (rc != NF_OK) return rc;
    // NF_GRAD_PATH_GEMM: the gate records live in a buffer of the handle's workspace set: one per call in flight, grown only by a call
    // that needs more than any earlier one (nf_reserve_grad_workspace sizes it up front); everything else is enqueued
    const bool gemm = h->grad_path == NF_GRAD_PATH_GEMM;
    nf_handle::Workspace *wsp = nullptr;
    if (gemm && (rc = ws_acquire(h, grad_workspace_bytes(h, B), (hipStream_t)stream, &wsp)) != NF_OK) return rc;
    const hipError_t e = grad_launch(h, h->gprog, a, h->grad_n_cpl, wsp ? wsp->p : nullptr, wsp ? wsp->bytes : 0, (hipStream_t)stream);
    if (gemm) ws_release(h, wsp, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, gemm ? "nf_nll_grad launch (GEMM)" : "nf_nll_grad launch");
    return NF_OK;
}

// ---- vector-Jacobian product of sampling: d L / d y, d L / d eps, d L / d temp (nf_sample_grad.hip, nf_sample_grad_wide.hip) ----
int nf_sample_vjp_supported(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params)
{
    Built b;
    int rc = build_program(cfg, layers, params, n_params, 0, b);
    if (rc != NF_OK) return rc;
    return sample_vjp_support(cfg, b);
}

// ---- nf_sample_vjp on tiles (NF_CFG_SVJP_TILED; nf_device.h, "gradient tiles", NfSampleGradTileLaunch) ----
// Sampling-order segment j of a tiled call is segment S - 1 - j of the gradient plan: op i of the NLL program is op n - 1 - i of the
// sampling program.  Its forward launch runs on the sampling direction's own tiles (tile_h x tile_w, halo 2 per coupling), as
// grad_fwd_seg's.
static Built::TileSeg svjp_fwd_seg(const nf_handle *h, int j)
{
    const int S = (int)h->grad_segs.size(), n = h->gprog.n_ops;
    const Built::TileSeg &g = h->grad_segs[S - 1 - j];
    Built::TileSeg f;
    f.op0 = n - g.op1;
    f.op1 = n - g.op0;
    f.halo = g.halo / kGradSegs.halo_per_cpl * kFwdSegs.halo_per_cpl;
    f.ny = nf_tile_count(h->cfg.height, h->rev.tile_h, f.halo);
    f.nx = nf_tile_count(h->cfg.width, h->rev.tile_w, f.halo);
    return f;
}

// scratch of one call: the tile sums of the NLL-last segment's launch (gtemp), the S - 1 tensors between two segments, two gradient
// tensors (ping-pong).  NF_SVJP_PATH_GEMM: the gate records of the launch's workgroups — one per WORKGROUP, not per patch, the count
// from the function the launcher takes its grid from (what grad_workspace_bytes gives for nf_nll_grad on the same handle)
static size_t svjp_workspace_bytes(const nf_handle *h, int64_t B)
{
    if (h->svjp_rc != NF_OK || B <= 0) return 0;
    if (h->svjp_path == NF_SVJP_PATH_GEMM)
        return round_up_256((size_t)nf_grad_gemm_groups(B, h->n_cu) * nfgg_gate_halves(h->cfg.height * h->cfg.width, h->gprog.width, h->grad_n_cpl) * sizeof(uint16_t));
    if (h->svjp_path != NF_SVJP_PATH_TILED) return 0;
    const int S = (int)h->grad_segs.size();
    const Built::TileSeg &last = h->grad_segs[S - 1];
    return round_up_256((size_t)B * last.ny * last.nx * sizeof(float)) + grad_img_bytes(h, B) * (size_t)(S - 1 + (S - 1 < 2 ? S - 1 : 2));
}

// Forward: the tiled launches of nf_sample cut at the gradient plan's boundaries, every tensor between two segments kept; the
// sampling-last one runs only for x_out.  Backward: one launch of nf_sample_grad_kernel<.., TILED> per segment in NLL order, first to
// last; segment s starts from the tensor kept behind it (the NLL-last one from eps * temp), takes the gradient segment s - 1 stored
// (the first one gx_in) and stores core windows — to the other of two scratch tensors, or (the NLL-last one) geps_out = temp g and
// its tile sums of g eps, which nf_tile_sum_kernel adds up per image.  gy_out: the first launch whose segment has an SDN-kind op
// stores it, later ones add to it.  Everything is enqueued on `st`.
static int sample_vjp_tiled(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base, float temp, int64_t B,
                            const nf_cond_row &r, const nf_cond_row *rows, const float *gx_in, float *x_out, float *gy_out, float *geps_out,
                            float *gtemp_out, hipStream_t st)
{
    const int S = (int)h->grad_segs.size(), H = h->cfg.height, W = h->cfg.width;
    const int fpath = select_path(h, 1);
    if (h->rev.lay[fpath].prog.n_ops != h->gprog.n_ops) return fail(NF_EINVAL, "nf_sample_vjp: the sampling program does not mirror the gradient program");
    NfTileParts tp;
    memset(&tp, 0, sizeof(tp));
    tp.n_seg = S;
    Built::TileSeg fseg[NF_MAX_TILE_SEGS];
    for (int j = 0; j < S; ++j) {
        fseg[j] = svjp_fwd_seg(h, j);
        tp.nt[j] = fseg[j].ny * fseg[j].nx;
        const int64_t most = std::max<int64_t>(tp.nt[j], (int64_t)h->grad_segs[j].ny * h->grad_segs[j].nx);
        if (B > (INT64_MAX / 64) / most) return fail(NF_EINVAL, "B too large");
    }
    const bool back = gy_out || geps_out || gtemp_out;
    nf_handle::Workspace *wsp = nullptr;
    const int rc = ws_acquire(h, svjp_workspace_bytes(h, B), st, &wsp);
    if (rc != NF_OK) return rc;
    const size_t img_bytes = grad_img_bytes(h, B);
    const int nt_last = h->grad_segs[S - 1].ny * h->grad_segs[S - 1].nx;
    char *q = wsp->p;
    float *const sums = reinterpret_cast<float *>(q);
    q += round_up_256((size_t)B * nt_last * sizeof(float));
    float *kept[NF_MAX_TILE_SEGS + 1] = {}, *gbuf[2] = {nullptr, nullptr};   // kept[s]: the tensor in front of NLL segment s (s = 1 .. S - 1)
    for (int s = 1; s < S; ++s, q += img_bytes) kept[s] = reinterpret_cast<float *>(q);
    for (int i = 0; i < 2 && i < S - 1; ++i, q += img_bytes) gbuf[i] = reinterpret_cast<float *>(q);

    hipError_t e = hipSuccess;
    const int n_fwd = x_out ? S : S - 1;   // the sampling-last segment's forward launch only forms x
    if (n_fwd > 0) {
        NfLaunch a;
        memset(&a, 0, sizeof(a));
        a.in = eps;
        a.y = y;
        a.B = B;
        a.patch_base = patch_index_base;
        a.seed = seed;
        a.in_scale = temp;
        memcpy(a.cond_a, r.a, sizeof(r.a));
        memcpy(a.cond_b, r.b, sizeof(r.b));
        a.cond_rows = rows;
        a.flags = eps ? 0u : NF_K_PHILOX_IN;
        float *outs[NF_MAX_TILE_SEGS];
        for (int j = 0; j < S; ++j) outs[j] = j == S - 1 ? x_out : kept[S - 1 - j];
        e = launch_segments(h, 1, a, fseg, n_fwd, tp, nullptr, outs, st);
    }
    if (e == hipSuccess && back) {
        NfSampleGradTileLaunch a;
        memset(&a, 0, sizeof(a));
        a.params = h->d_grad;
        a.y = y;
        a.eps = eps;
        a.patch_base = patch_index_base;
        a.seed = seed;
        a.temp = temp;
        memcpy(a.cond_a, r.a, sizeof(r.a));
        memcpy(a.cond_b, r.b, sizeof(r.b));
        a.cond_rows = rows;
        a.H = H < NF_GRAD_TILE ? H : NF_GRAD_TILE;
        a.W = W < NF_GRAD_TILE ? W : NF_GRAD_TILE;
        a.img_H = H;
        a.img_W = W;
        a.gate_words = nf_grad_gate_words(h->grad_seg_cpl, h->gprog.width);
        bool gy_written = false;
        for (int s = 0; s < S && e == hipSuccess; ++s) {
            const Built::TileSeg &g = h->grad_segs[s];
            NfProgram sp;
            memset(&sp, 0, sizeof(sp));
            sp.width = h->gprog.width;
            sp.n_ops = g.op1 - g.op0;
            memcpy(sp.ops, h->gprog.ops + g.op0, sizeof(NfOp) * (size_t)sp.n_ops);
            NfSampleGradTileLaunch t = a;
            t.last_cpl = -1;
            bool sdn = false;
            for (int i = 0; i < sp.n_ops; ++i) {
                if (sp.ops[i].type == NF_OP_COUPLING_FWD) {
                    t.last_cpl = i;
                    ++t.n_cpl;
                }
                sdn = sdn || sp.ops[i].type == NF_OP_SDN_DIV;
            }
            const bool last = s == S - 1;
            t.B = B * g.ny * g.nx;
            t.tile_ny = g.ny;
            t.tile_nx = g.nx;
            t.tile_halo = g.halo;
            t.z_in = last ? nullptr : kept[s + 1];
            t.g_in = s == 0 ? gx_in : gbuf[(s - 1) & 1];
            t.g_out = last ? nullptr : gbuf[s & 1];
            t.geps_out = last ? geps_out : nullptr;
            t.tile_sum = last && gtemp_out ? sums : nullptr;
            // a model without an SDN-kind op: the last launch stores the zeros
            const bool wr = gy_out && (sdn || (last && !gy_written));
            t.gy_out = wr ? gy_out : nullptr;
            t.tflags = wr && gy_written ? NF_GT_GY_ACC : 0u;
            gy_written = gy_written || wr;
            if (last && !t.geps_out && !t.tile_sum && !t.gy_out) break;   // nothing left to store
            e = nf_launch_sample_grad_tiled(sp, t, h->grad_seg_cpl, h->n_cu, st);
        }
        if (e == hipSuccess && gtemp_out) e = nf_launch_tile_sum(sums, nt_last, B, gtemp_out, st);
    }
    ws_release(h, wsp, st);
    if (e != hipSuccess) return fail_hip(e, "nf_sample_vjp launch (tiles)");
    return NF_OK;
}

int nf_reserve_sample_vjp_workspace(nf_handle *h, int64_t B, int32_t calls_in_flight)
{
    if (!h || B < 0 || calls_in_flight < 1 || calls_in_flight > 64) return fail(NF_EINVAL, "bad argument");
    return reserve_workspace(h, svjp_workspace_bytes(h, B), calls_in_flight);
}

int nf_sample_vjp_path(const nf_handle *h)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (h->svjp_rc != NF_OK) return fail(h->svjp_rc, "%s", h->svjp_why.c_str());
    return h->svjp_path;
}

int nf_sample_vjp(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base, float temp, int64_t B,
                  const nf_cond *cond, const nf_cond_row *rows, const float *gx_in, float *x_out, float *gy_out, float *geps_out,
                  float *gtemp_out, void *stream)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (h->svjp_rc != NF_OK) return fail(h->svjp_rc, "%s", h->svjp_why.c_str());
    if (B < 0) return fail(NF_EINVAL, "B must be >= 0");
    if ((cond != nullptr) == (rows != nullptr)) return fail(NF_EINVAL, "nf_sample_vjp: exactly one of cond / rows must be given");
    if (B > 0 && !gx_in) return fail(NF_EINVAL, "gx_in is NULL");
    if (h->rev.has_sdn && B > 0 && !y) return fail(NF_EINVAL, "model has a signal-dependent layer but y is NULL");
    if (!y && gy_out) return fail(NF_EINVAL, "gy_out must be NULL when y is");
    if (!aligned16(y) || !aligned16(eps) || !aligned16(gx_in) || !aligned16(x_out) || !aligned16(gy_out) || !aligned16(geps_out))
        return fail(NF_EINVAL, "y, eps, gx_in, x_out, gy_out and geps_out must be 16-byte aligned (every pixel is one float4 access)");
    nf_cond_row r;
    memset(&r, 0, sizeof(r));
    if (rows) {
        int rc = check_rows(h, rows, B);
        if (rc != NF_OK) return rc;
    } else {
        int rc = cond_row_of(h->rev, h->cfg.height, h->cfg.width, 1, cond, r);
        if (rc != NF_OK) return rc;
    }
    if (B == 0) return NF_OK;
    if (h->svjp_path == NF_SVJP_PATH_TILED) {
        NfDeviceGuard guard;
        int rc = guard.enter(h->device);
        if (rc != NF_OK) return rc;
        return sample_vjp_tiled(h, y, eps, seed, patch_index_base, temp, B, r, rows, gx_in, x_out, gy_out, geps_out, gtemp_out, (hipStream_t)stream);
    }
    NfSampleGradLaunch a;
    memset(&a, 0, sizeof(a));
    a.params = h->d_grad;
    a.y = y;
    a.eps = eps;
    a.gx_in = gx_in;
    a.x_out = x_out;
    a.gy_out = gy_out;
    a.geps_out = geps_out;
    a.gtemp_out = gtemp_out;
    a.B = B;
    a.patch_base = patch_index_base;
    a.seed = seed;
    a.temp = temp;
    memcpy(a.cond_a, r.a, sizeof(r.a));
    memcpy(a.cond_b, r.b, sizeof(r.b));
    a.cond_rows = rows;
    a.H = h->cfg.height;
    a.W = h->cfg.width;
    a.last_cpl = h->svjp_last_cpl;
    a.n_cpl = h->grad_n_cpl;
    const bool wide = h->svjp_path == NF_SVJP_PATH_WIDE32, gemm = h->svjp_path == NF_SVJP_PATH_GEMM;
    a.gate_words = gemm ? 0 : wide ? nfgw_tpw(a.H) * h->grad_n_cpl : nf_grad_gate_words(h->grad_n_cpl, h->gprog.width);   // (GEMM: device scratch)
    NfDeviceGuard guard;
    int rc = guard.enter(h->device);
    if (rc != NF_OK) return rc;
    if (gemm) {
        // the gate records live in a buffer of the handle's workspace set, as nf_nll_grad's on NF_GRAD_PATH_GEMM: one per call in
        // flight, grown only by a call that needs more than any earlier one (nf_reserve_sample_vjp_workspace sizes it up front)
        nf_handle::Workspace *wsp = nullptr;
        if ((rc = ws_acquire(h, svjp_workspace_bytes(h, B), (hipStream_t)stream, &wsp)) != NF_OK) return rc;
        const hipError_t eg = nf_launch_sample_grad_gemm(h->gprog, a, h->n_cu, wsp ? wsp->p : nullptr, wsp ? wsp->bytes : 0, (hipStream_t)stream);
        ws_release(h, wsp, (hipStream_t)stream);
        if (eg != hipSuccess) return fail_hip(eg, "nf_sample_vjp launch (GEMM)");
        return NF_OK;
    }
    const hipError_t e = wide ? nf_launch_sample_grad_wide(h->gprog, a, h->n_cu, (hipStream_t)stream)
                              : nf_launch_sample_grad(h->gprog, a, h->n_cu, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "nf_sample_vjp launch");
    return NF_OK;
}

// ---- batch-statistics mode (is_training=True graphs: layers.py:386-398) ----
// The normalisation of every coupling CNN uses the moments of the CURRENT call's B patches, which couples all
// patches: the moments of coupling c depend on the outputs of the couplings before it under THEIR batch moments.
// The call therefore walks the couplings in execution order with the tensor in front of each one RESIDENT in HBM
// (T_0 = the caller's input, T_c = the output of coupling c-1 in one of two scratch buffers); per coupling c
//   launch A_c : [segment c-1 = the layers after coupling c-2 up to coupling c-1, with its moments; STORE T_c;] segment c, statistics of its l_1
//   launch B_c : the same segment from T_c with BN_1 folded, statistics of its l_2
// each followed by a one-workgroup kernel that turns the sums into moments and re-folds the layer IN PLACE on a
// device-resident working copy of the parameter block (which starts as the identity-normalised model), and finally
// one fused pass over the LAST segment (+ the layers behind the last coupling) from the last resident tensor: every
// earlier segment already ran in its final form in the launch that stored the tensor behind it, and the log-det it
// contributed travels with that tensor (NfLaunch::ld_carry, one float per thread of the patch's workgroup).  2 short launches per coupling instead of
// re-running the whole prefix, no host round trip until the moments are copied out at the end.
//
// Two routes run this schedule (bs_route; the third, NF_BS_ROUTE_TRAINER, is run_batchstats_wide): ONE walker, bs_walk, holds the
// loops, the input choice, the resident-tensor ping-pong, the log-det carry and the moments; a route description (BsScalarRoute /
// BsMfma4Route) says which layout's programs and parameter block a launch reads, where a pass puts its sums, and what becomes of
// them — a finaliser kernel on the scalar-weight route, the "pending fix" in the prologue of the next launch on the width-4 one.

// The launches of the schedule over ONE kernel layout (lay[NF_PATH_SCALAR] or lay[NF_PATH_MFMA4] of the identity-normalised model)
struct BsProgs {
    std::vector<NfProgram> A, B;      // per coupling: the two statistics launches
    NfProgram F;                      // the final launch: the last segment + everything behind it (the whole program with < 2 couplings)
};

struct BsPlan {
    bool ready = false;
    Built ident;                      // the model folded with an identity normalisation in every coupling CNN
    DevBuf<float> d_ident[2];         // ... on the device, [NF_PATH_SCALAR] / [NF_PATH_MFMA4] (empty where the model has no such layout)
    BsProgs progs[2];                 // same index
    std::vector<int> cpl_ops;         // op index of every coupling in ident's programs, execution order
    std::vector<int> cpl_row;         // its row in moments_out (NLL layer order)
    std::vector<float> shift;         // [coupling in NLL layer order][2][width]: the running means the statistics are taken around
};
static_assert(NF_PATH_SCALAR == 0 && NF_PATH_MFMA4 == 1, "BsPlan indexes its two layouts by path");

struct nf_bs_state {
    BsPlan plan[2];
    DevBuf<float> work;                // scalar-weight route: the working copy of the parameter block, re-folded in place
    DevBuf<double> stats;              // ... its one [NF_STATS_SLOTS][2 w] block of sums (the finaliser zeroes it again)
    DevBuf<float> work_mc[2];          // width-4 route: the launches ping-pong between two working copies (matrix-core layout)
    DevBuf<double> stats_mc;           // ... one [NF_STATS_SLOTS][8] block per statistics pass
    DevBuf<float> mom;                 // [couplings][4][w]
    DevBuf<float> T[2];                // the resident tensors
    DevBuf<float> carry;               // [B][1024] per-thread log-det of the segments behind the resident tensor
    nf_trainer *wide = nullptr;        // the layer-by-layer evaluator on the trainer's GEMM path (nf_bs_wide_*), where the passes above do not reach
    ~nf_bs_state()
    {
        if (wide) (void)nf_trainer_destroy(wide);
    }
};

static int bs_build_plan(nf_handle *h, int direction, BsPlan &P)
{
    // unit-scale normalisation in every coupling: var 1 - eps -> scale exactly 1.  The MEAN stays the stored running mean:
    // the statistics passes then see activations centred near zero, so that their one-pass sum / sum-of-squares does not
    // cancel when a channel's mean is large against its spread (shipped model: mean^2 / var up to 400); the re-fold
    // B <- (B - mean') * scale is unchanged, and the reported batch mean is mean' + running mean.
    std::vector<float> p = h->raw;
    int n_cpl = 0;
    P.shift.clear();
    for (int i = 0; i < h->cfg.n_layers; ++i) {
        const nf_layer_desc &L = h->layers[i];
        if (L.type != NF_LAYER_COUPLING) continue;
        ++n_cpl;
        const int w = L.width, wk = h->fwd.lay[NF_PATH_SCALAR].prog.width;   // width of the variables / of the kernels' layout (zero-padded channels:
                                                          // activation 0 on every pixel, batch moments 0, weights and bias stay 0)
        float *lp = p.data() + L.param_offset;
        float *mv[4] = {lp + 19 * w, lp + 20 * w, lp + 22 * w + w * w, lp + 23 * w + w * w};
        P.shift.insert(P.shift.end(), mv[0], mv[0] + w);
        P.shift.insert(P.shift.end(), (size_t)(wk - w), 0.0f);
        P.shift.insert(P.shift.end(), mv[2], mv[2] + w);
        P.shift.insert(P.shift.end(), (size_t)(wk - w), 0.0f);
        for (int j = 0; j < w; ++j) mv[1][j] = mv[3][j] = (float)(1.0 - kBnEps);
    }
    int rc = build_program(&h->cfg, h->layers.data(), p.data(), p.size(), direction, P.ident);
    if (rc != NF_OK) return rc;
    const NfProgram &prog = P.ident.lay[NF_PATH_SCALAR].prog;
    P.cpl_ops.clear();
    for (int i = 0; i < prog.n_ops; ++i)
        if (prog.ops[i].type == NF_OP_COUPLING_FWD || prog.ops[i].type == NF_OP_COUPLING_REV) P.cpl_ops.push_back(i);
    if ((int)P.cpl_ops.size() != n_cpl) return fail(NF_EINVAL, "internal: batch-statistics plan mismatch");
    P.cpl_row.resize(n_cpl);
    for (int c = 0; c < n_cpl; ++c) P.cpl_row[c] = direction == 0 ? c : n_cpl - 1 - c;
    // A launch = a list of op indices into the full program (every layout has the same op sequence: build_layout) and kStore for
    // the NF_OP_STORE behind a re-run segment; built once, then materialised against each layout's program, whose offsets it takes.
    const int kStore = -1;
    typedef std::vector<int> Seg;
    auto append = [](Seg &s, int first, int last) {
        for (int i = first; i <= last; ++i) s.push_back(i);
    };
    auto seg_first = [&](int c) { return c <= 0 ? 0 : P.cpl_ops[c - 1] + 1; };   // segment c = the layers after coupling c-1 up to and including coupling c
    std::vector<Seg> segA(n_cpl), segB(n_cpl);
    Seg segF;
    for (int c = 0; c < n_cpl; ++c) {
        if (c > 0) {   // segment c-1, now with its moments
            append(segA[c], seg_first(c - 1), P.cpl_ops[c - 1]);
            segA[c].push_back(kStore);
        }
        append(segA[c], seg_first(c), P.cpl_ops[c]);
        append(segB[c], seg_first(c), P.cpl_ops[c]);
        if ((int)segA[c].size() > NF_MAX_OPS) return fail(NF_EINVAL, "too many layers for the batch-statistics plan");
    }
    append(segF, seg_first(n_cpl - 1), prog.n_ops - 1);
    if ((int)segF.size() > NF_MAX_OPS) return fail(NF_EINVAL, "too many layers for the batch-statistics plan");
    for (int path : {NF_PATH_SCALAR, NF_PATH_MFMA4}) {
        const Layout &lay = P.ident.lay[path];
        if (lay.block.empty()) continue;
        auto materialise = [&](const Seg &s) {
            NfProgram out;
            memset(&out, 0, sizeof(out));
            out.width = lay.prog.width;
            for (int i : s) {
                if (i == kStore) out.ops[out.n_ops].type = NF_OP_STORE;
                else out.ops[out.n_ops] = lay.prog.ops[i];
                ++out.n_ops;
            }
            return out;
        };
        BsProgs &G = P.progs[path];
        G.A.clear();
        G.B.clear();
        for (int c = 0; c < n_cpl; ++c) {
            G.A.push_back(materialise(segA[c]));
            G.B.push_back(materialise(segB[c]));
        }
        G.F = materialise(segF);
        hipError_t e;
        if ((e = P.d_ident[path].reserve(lay.block.size())) != hipSuccess ||
            (e = hipMemcpy(P.d_ident[path].ptr, lay.block.data(), lay.block.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
            return fail_hip(e, "batch-statistics plan upload");
    }
    P.ready = true;
    return NF_OK;
}

// all-reduce the `nvals` slotted sums of one statistics pass over the ranks (no-op without nf_set_sync): the totals come
// back as slot 0, so the consumer — the next launch's prologue or nf_bs_finalize — needs no other change than n x world
static int bs_sync(nf_handle *h, double *stats, int nvals, hipStream_t st)
{
    if (!h->sync_fn || h->sync_world < 2) return NF_OK;
    if (nvals > 64) return fail(NF_EINVAL, "cross-rank batch statistics cover coupling widths up to 32");
    hipError_t e = nf_launch_stats_compact(stats, nvals, h->sync_buf, st);
    if (e != hipSuccess) return fail_hip(e, "batch-statistics compaction");
    const int rc = h->sync_fn(h->sync_user, h->sync_buf, (int64_t)nvals, (void *)st);
    if (rc != 0) return fail(NF_EINVAL, "the all-reduce callback of nf_set_sync failed (status %d)", rc);
    if ((e = nf_launch_stats_scatter(stats, nvals, h->sync_buf, st)) != hipSuccess) return fail_hip(e, "batch-statistics scatter");
    return NF_OK;
}

// Where the statistics passes of the fused kernels do not reach — coupling widths beyond 32 (sidd/ArgParser.py:43 defaults to 512),
// and patches beyond the scalar-weight kernel's two LDS tiles at widths 5 .. 32 (64x64 at the paper's width 32) — the call is a
// layer-by-layer walk on the trainer's matrix-core GEMM path (nf_train.hip: nf_bs_wide_run): same moments, same outputs, one
// resident tensor; the evaluator is created on first use and grows with B.
static int run_batchstats_wide(nf_handle *h, int direction, const NfLaunch &a, const nf_cond *cond, float *moments_out, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(h->bs_mu);   // one evaluator per handle: calls serialise
    if (!h->bs) h->bs = new (std::nothrow) nf_bs_state();
    if (!h->bs) return fail(NF_ENOMEM, "out of host memory");
    nf_bs_state &S = *h->bs;
    int64_t cap = a.B;
    if (S.wide && nf_bs_wide_capacity(S.wide) < a.B) {
        // grow geometrically: a caller that ramps its batch size pays O(log B) re-allocations of the evaluator's tensors, not one per step
        cap = std::max<int64_t>(a.B, 2 * nf_bs_wide_capacity(S.wide));
        (void)nf_trainer_destroy(S.wide);
        S.wide = nullptr;
    }
    if (!S.wide) {
        nf_config cfg = h->cfg;
        cfg.device = h->device;
        int rc = nf_bs_wide_create(&cfg, h->layers.data(), h->raw.data(), h->raw.size(), cap, &S.wide);
        if (rc != NF_OK && cap > a.B) rc = nf_bs_wide_create(&cfg, h->layers.data(), h->raw.data(), h->raw.size(), a.B, &S.wide);   // (no room for the head-room)
        if (rc != NF_OK) return rc;
    }
    nf_bs_wide_args w;
    memset(&w, 0, sizeof(w));
    w.direction = direction;
    w.in = (a.flags & NF_K_PHILOX_IN) ? nullptr : a.in;
    w.y = a.y;
    w.B = a.B;
    w.cond = cond;
    w.seed = a.seed;
    w.patch_base = a.patch_base;
    w.in_scale = a.in_scale;
    w.out = a.out;
    w.nll_out = a.nll_out;
    w.sd_out = a.sd_out;
    w.ld_out = a.ld_out;
    w.sums = a.sums;
    w.prior = (a.flags & NF_K_PRIOR) != 0;
    w.moments_out = moments_out;
    w.sync_fn = h->sync_fn;
    w.sync_user = h->sync_user;
    w.sync_buf = h->sync_buf;
    w.sync_world = h->sync_world;
    return nf_bs_wide_run(S.wide, w, st);
}

// ---- what bs_walk asks of a route ----
// A further route adds such a struct, its case in run_batchstats and its condition in bs_route; bs_walk stays as it is.
// (Virtual calls, one per launch: no allocation, and nothing next to the launch itself.)
struct BsRoute {
    nf_handle *h;
    nf_bs_state &S;
    const BsPlan &P;
    hipStream_t st;
    const int path;    // the kernel layout: which BsProgs / d_ident of the plan the launches read
    const int w;       // its coupling width
    const double n;    // values per channel and pass
    int nt = 1;        // workgroups a patch is cut into
    BsRoute(nf_handle *h_, nf_bs_state &S_, const BsPlan &P_, hipStream_t st_, int path_, double n_)
        : h(h_), S(S_), P(P_), st(st_), path(path_), w(P_.ident.lay[path_].prog.width), n(n_)
    {
    }
    virtual int prepare(int n_cpl) = 0;                                   // its own scratch, and what it puts on the stream in front of the first launch
    virtual double *stats_of(int c, int stage) const = 0;                 // the block of sums of that pass
    virtual hipError_t launch(const NfProgram &prog, NfLaunch &s) = 0;    // one launch on its kernel: the parameter block and whatever else it adds to a launch
    virtual int after_pass(int c, int stage, const NfLaunch &s, float *mom) = 0;   // what becomes of the sums of the pass just launched (`mom`: the coupling's [4][w] moments)
    virtual int final(const NfProgram &prog, NfLaunch &a) = 0;            // the last launch, with the outputs of the call

protected:
    ~BsRoute() = default;
};

struct BsScalarRoute final : BsRoute {
    BsScalarRoute(nf_handle *h_, nf_bs_state &S_, const BsPlan &P_, hipStream_t st_, double n_) : BsRoute(h_, S_, P_, st_, NF_PATH_SCALAR, n_) {}
    int prepare(int) override
    {
        hipError_t e;
        const size_t nw = P.ident.lay[path].block.size();
        if ((e = S.work.reserve(nw)) != hipSuccess) return fail_hip(e, "hipMalloc(batch-statistics parameters)");
        if ((e = S.stats.reserve(NF_STATS_SLOTS * 64)) != hipSuccess) return fail_hip(e, "hipMalloc(batch-statistics accumulators)");
        if ((e = hipMemcpyAsync(S.work.ptr, P.d_ident[path].ptr, nw * sizeof(float), hipMemcpyDeviceToDevice, st)) != hipSuccess ||
            (e = hipMemsetAsync(S.stats.ptr, 0, NF_STATS_SLOTS * 2 * (size_t)w * sizeof(double), st)) != hipSuccess)
            return fail_hip(e, "batch-statistics set-up");
        return NF_OK;
    }
    double *stats_of(int, int) const override { return S.stats.ptr; }
    hipError_t launch(const NfProgram &prog, NfLaunch &s) override
    {
        s.params = S.work.ptr;
        s.n_params = 0;
        return nf_launch_flow(prog, s, h->n_cu, st, false);
    }
    // a one-workgroup kernel turns the sums into moments and re-folds the layer in place
    int after_pass(int c, int stage, const NfLaunch &, float *mom) override
    {
        float *blk = S.work.ptr + P.ident.lay[path].prog.ops[P.cpl_ops[c]].off;
        float *Wm = blk + (stage == 1 ? nf_cpl_off_W1(w) : nf_cpl_off_W2(w));
        float *Bv = blk + (stage == 1 ? nf_cpl_off_B1(w) : nf_cpl_off_B2(w));
        const hipError_t e = nf_launch_bs_finalize(S.stats.ptr, w, n, Wm, stage == 1 ? 18 : w, Bv, mom + (stage == 1 ? 0 : 2 * w),
                                                   mom + (stage == 1 ? w : 3 * w), st);
        return e == hipSuccess ? NF_OK : fail_hip(e, "batch-statistics finalise");
    }
    int final(const NfProgram &prog, NfLaunch &a) override
    {
        const hipError_t e = launch(prog, a);
        return e == hipSuccess ? NF_OK : fail_hip(e, "batch-statistics final launch");
    }
};

// Width 4: every launch on the matrix-core kernel, the re-fold fused into the consumer's prologue.  Launch k gathers the sums of
// pass k into its own block of `stats_mc`; launch k+1 (every workgroup, in LDS) turns them into moments and rescales the layer,
// workgroup 0 writes the patched image to the OTHER working copy, which launch k+2 reads.  2 launches per coupling + the final
// fused pass, nothing else on the stream.  Images beyond 64x64 (nf_device.h, "overlapping tiles"): every launch tiled with ONE halo
// for the whole call — 3 = the deepest launch (re-run coupling c-1, then l_1 of coupling c for its statistics) — so that the tile
// grid, and with it the per-thread log-det carry, is the same in every launch.
struct BsMfma4Route final : BsRoute {
    static constexpr int halo = 3;
    const int64_t B;   // images of the call
    const int direction;
    const bool tiled;
    int ny = 1, nx = 1;
    const float *cur = nullptr;   // parameter block the next launch reads
    int nbuf = 0;                 // working copy the next fix writes
    // the fix a launch has to apply = the pass of the launch before it
    const double *pend_stats = nullptr;
    int pend_off = 0, pend_stage = 0;
    float *pend_mom = nullptr;

    BsMfma4Route(nf_handle *h_, nf_bs_state &S_, const BsPlan &P_, hipStream_t st_, double n_, int64_t B_, int direction_)
        : BsRoute(h_, S_, P_, st_, NF_PATH_MFMA4, n_), B(B_), direction(direction_), tiled(h_->fwd.tiled)
    {
        if (tiled) {
            ny = nf_tile_count(h->cfg.height, h->fwd.tile_h, halo);
            nx = nf_tile_count(h->cfg.width, h->fwd.tile_w, halo);
            nt = ny * nx;
        }
    }
    int prepare(int n_cpl) override
    {
        hipError_t e;
        const size_t nw = P.ident.lay[path].block.size(), nstats = 2 * (size_t)n_cpl * NF_STATS_SLOTS * 8;
        if ((e = S.work_mc[0].reserve(nw)) != hipSuccess || (e = S.work_mc[1].reserve(nw)) != hipSuccess)
            return fail_hip(e, "hipMalloc(batch-statistics parameters)");
        if ((e = S.stats_mc.reserve(nstats)) != hipSuccess) return fail_hip(e, "hipMalloc(batch-statistics accumulators)");
        if ((e = hipMemsetAsync(S.stats_mc.ptr, 0, nstats * sizeof(double), st)) != hipSuccess) return fail_hip(e, "batch-statistics set-up");
        cur = P.d_ident[path].ptr;
        return NF_OK;
    }
    double *stats_of(int c, int stage) const override { return S.stats_mc.ptr + (size_t)(2 * c + stage - 1) * NF_STATS_SLOTS * 8; }
    hipError_t launch(const NfProgram &prog, NfLaunch &s) override
    {
        s.params = cur;
        s.n_params = (int32_t)P.ident.lay[path].block.size();
        s.flags |= NF_K_BATCHSTATS;
        if (tiled) {   // every "patch" of the launch is one tile of an image (tensors stay image-shaped)
            s.flags |= NF_K_TILED;
            s.img_H = h->cfg.height;
            s.img_W = h->cfg.width;
            s.H = h->fwd.tile_h;
            s.W = h->fwd.tile_w;
            s.tile_ny = ny;
            s.tile_nx = nx;
            s.tile_halo = halo;
            s.B = B * nt;
        }
        s.fix_stats = pend_stats;
        s.fix_n = n;
        s.fix_off = pend_off;
        s.fix_stage = pend_stage;
        s.fix_mom_out = pend_mom;
        s.fix_params_out = pend_stats ? S.work_mc[nbuf].ptr : nullptr;
        const hipError_t e = nf_launch_flow(prog, s, h->n_cu, st, true);
        if (pend_stats) {
            cur = S.work_mc[nbuf].ptr;
            nbuf ^= 1;
        }
        return e;
    }
    int after_pass(int c, int stage, const NfLaunch &s, float *mom) override
    {
        pend_stats = s.stats;
        pend_off = P.ident.lay[path].prog.ops[P.cpl_ops[c]].off;
        pend_stage = stage;
        pend_mom = mom + (stage == 1 ? 0 : 2 * w);
        return NF_OK;
    }
    int final(const NfProgram &prog, NfLaunch &a) override
    {
        hipError_t e;
        if (!tiled) return (e = launch(prog, a)) == hipSuccess ? NF_OK : fail_hip(e, "batch-statistics final launch");
        // the final launch leaves per-tile sums; one more kernel forms the per-image results (as launch_tiled)
        const bool want = direction == 0 && (a.nll_out || a.sd_out || a.ld_out || a.sums);
        NfLaunch f = a;
        f.nll_out = f.sd_out = f.ld_out = nullptr;
        f.sums = nullptr;
        float *part = nullptr;
        if (want && (e = hipMallocAsync((void **)&part, (size_t)B * nt * 4 * sizeof(float), st)) != hipSuccess)
            return fail_hip(e, "hipMallocAsync(tile sums)");
        f.tile_part = part;
        e = launch(prog, f);
        if (e == hipSuccess && want) {
            NfTileParts tp;
            memset(&tp, 0, sizeof(tp));
            tp.n_seg = 1;
            tp.nt[0] = nt;
            e = nf_launch_tile_combine(part, tp, B, (double)h->cfg.height * h->cfg.width * kC, a.ld_const, nullptr, a.flags, a.nll_out,
                                       a.sd_out, a.ld_out, a.sums, st);
        }
        if (part) {
            const hipError_t e2 = hipFreeAsync(part, st);
            if (e == hipSuccess) e = e2;
        }
        return e == hipSuccess ? NF_OK : fail_hip(e, "batch-statistics final launch");
    }
};

// The schedule: per coupling two statistics passes, then the final pass, then the moments.
static int bs_walk(BsRoute &R, int direction, NfLaunch &a, float *moments_out)
{
    nf_handle *const h = R.h;
    nf_bs_state &S = R.S;
    const BsPlan &P = R.P;
    const hipStream_t st = R.st;
    const BsProgs &G = P.progs[R.path];
    const int n_cpl = (int)P.cpl_ops.size();
    const int w = R.w, wr = h->fwd.raw_width;   // the kernels' rows of moments are [4][w]; moments_out's [4][wr] (zero-padded widths)
    hipError_t e;
    int rc;
    if ((e = S.mom.reserve((size_t)std::max(n_cpl, 1) * 4 * 32)) != hipSuccess) return fail_hip(e, "hipMalloc(batch-statistics moments)");
    if (n_cpl > 1 && ((e = S.T[0].reserve((size_t)a.B * a.H * a.W * 4)) != hipSuccess || (e = S.T[1].reserve((size_t)a.B * a.H * a.W * 4)) != hipSuccess))
        return fail_hip(e, "hipMalloc(batch-statistics scratch tensors)");
    // the log-det only matters to the outputs that contain it
    const bool carry = n_cpl > 1 && (a.nll_out || a.ld_out || a.sums);
    if (carry && (e = S.carry.reserve((size_t)a.B * R.nt * 1024)) != hipSuccess) return fail_hip(e, "hipMalloc(batch-statistics log-det carry)");
    if ((rc = R.prepare(n_cpl)) != NF_OK) return rc;

    const float *const in0 = a.in;
    const float in_scale0 = a.in_scale;
    const uint32_t flags0 = a.flags;
    for (int c = 0; c < n_cpl; ++c) {
        float *mom = S.mom.ptr + (size_t)P.cpl_row[c] * 4 * w;
        for (int stage = 1; stage <= 2; ++stage) {
            const NfProgram &prog = stage == 1 ? G.A[c] : G.B[c];
            NfLaunch s = a;
            s.nll_out = s.sd_out = s.ld_out = nullptr;
            s.sums = nullptr;
            s.stats = R.stats_of(c, stage);
            s.stats_op = prog.n_ops - 1;
            s.stats_stage = stage;
            // launch A_c reads T_{c-1} (it re-runs coupling c-1), launch B_c reads T_c;  T_0 = the caller's input
            const int tin = stage == 1 ? (c > 0 ? c - 1 : 0) : c;
            const bool from_input = tin == 0;
            s.in = from_input ? in0 : S.T[tin & 1].ptr;
            s.in_scale = from_input ? in_scale0 : 1.0f;
            s.flags = from_input ? flags0 : (flags0 & ~(uint32_t)NF_K_PHILOX_IN);
            s.out = (stage == 1 && c > 0) ? S.T[c & 1].ptr : nullptr;
            if (carry && s.out) {
                s.flags |= NF_K_CARRY_OUT | (c > 1 ? NF_K_CARRY_ADD : 0u);
                s.ld_carry = S.carry.ptr;
            }
            if ((e = R.launch(prog, s)) != hipSuccess) return fail_hip(e, "batch-statistics launch");
            if ((rc = bs_sync(h, s.stats, 2 * w, st)) != NF_OK) return rc;
            if ((rc = R.after_pass(c, stage, s, mom)) != NF_OK) return rc;
        }
    }

    // final pass with the batch moments folded in: from the last resident tensor when there is one
    a.ld_const = a.ld_const + (direction == 0 ? P.ident.ld_const : 0.0);
    if (n_cpl > 1) {
        a.in = S.T[(n_cpl - 1) & 1].ptr;
        a.in_scale = 1.0f;
        a.flags &= ~(uint32_t)NF_K_PHILOX_IN;
        if (carry) {
            a.flags |= NF_K_CARRY_IN;
            a.ld_carry = S.carry.ptr;
        }
    }
    if ((rc = R.final(G.F, a)) != NF_OK) return rc;
    std::vector<float> mom_h((size_t)std::max(n_cpl, 1) * 4 * w);
    if (moments_out && n_cpl &&
        (e = hipMemcpyAsync(mom_h.data(), S.mom.ptr, (size_t)n_cpl * 4 * w * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail_hip(e, "batch-statistics moments readback");
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail_hip(e, "batch-statistics final sync");   // the scratch is reused
    if (moments_out && n_cpl) {
        for (int c = 0; c < n_cpl; ++c)              // [mean1, var1, mean2, var2][w] per coupling, NLL layer order, like P.shift
            for (int j = 0; j < w; ++j) {
                mom_h[(size_t)c * 4 * w + j] += P.shift[(size_t)c * 2 * w + j];
                mom_h[(size_t)c * 4 * w + 2 * w + j] += P.shift[(size_t)c * 2 * w + w + j];
            }
        for (int c = 0; c < n_cpl; ++c)              // the caller's rows hold the model's own channels
            for (int q = 0; q < 4; ++q)
                memcpy(moments_out + ((size_t)c * 4 + q) * wr, mom_h.data() + ((size_t)c * 4 + q) * w, (size_t)wr * sizeof(float));
    }
    return NF_OK;
}

static int run_batchstats(nf_handle *h, int direction, NfLaunch a, float *moments_out, hipStream_t st, const nf_cond *cond)
{
    if (h->cfg.flags & NF_CFG_FP16_CNN) return fail(NF_EINVAL, "batch-statistics mode is fp32 only");
    const int route = bs_route(h);   // (the trainer route has its own evaluator, lock and scratch)
    if (route == NF_BS_ROUTE_TRAINER) return run_batchstats_wide(h, direction, a, cond, moments_out, st);
    std::lock_guard<std::mutex> lock(h->bs_mu);   // one scratch per handle: calls serialise
    if (!h->bs) h->bs = new (std::nothrow) nf_bs_state();
    if (!h->bs) return fail(NF_ENOMEM, "out of host memory");
    nf_bs_state &S = *h->bs;
    BsPlan &P = S.plan[direction];
    if (!P.ready) {
        int rc = bs_build_plan(h, direction, P);
        if (rc != NF_OK) return rc;
    }
    const double n = (double)a.B * a.H * a.W * h->sync_world;   // with nf_set_sync the moments are over all ranks' patches
    switch (route) {
    case NF_BS_ROUTE_MFMA4: {
        BsMfma4Route R(h, S, P, st, n, a.B, direction);
        return bs_walk(R, direction, a, moments_out);
    }
    case NF_BS_ROUTE_SCALAR: {
        BsScalarRoute R(h, S, P, st, n);
        return bs_walk(R, direction, a, moments_out);
    }
    }
    return fail(NF_EINVAL, "internal: unknown batch-statistics route %d", route);
}

static void nf_bs_destroy(nf_bs_state *s) { delete s; }

int nf_nll_batchstats(nf_handle *h, const float *x, const float *y, int64_t B, const nf_cond *cond, float *nll_out,
                      float *sd_out, float *logdet_out, float *z_out, double *sums_out, uint32_t flags,
                      float *moments_out, void *stream)
{
    NfLaunch a;
    int rc = nll_args(h, x, y, B, cond, nll_out, sd_out, logdet_out, z_out, sums_out, flags, a);
    if (rc != NF_OK) return rc;
    if (B == 0) return fail(NF_EINVAL, "batch statistics of an empty batch are undefined");
    NfDeviceGuard guard;
    if ((rc = guard.enter(h->device)) != NF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (sums_out && !(flags & NF_ACCUMULATE)) {
        const size_t nb = (flags & NF_SUMS_WIDE) ? (size_t)NF_SUMS_SLOTS * NF_SUMS_STRIDE : 3;
        hipError_t e = hipMemsetAsync(sums_out, 0, nb * sizeof(double), st);
        if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(sums)");
    }
    return run_batchstats(h, 0, a, moments_out, st, cond);
}

int nf_sample_batchstats(nf_handle *h, const float *y, const float *eps, uint64_t seed, int64_t patch_index_base,
                         float temp, int64_t B, const nf_cond *cond, float *x_out, float *moments_out, void *stream)
{
    NfLaunch a;
    int rc = sample_args(h, y, eps, seed, patch_index_base, temp, B, cond, x_out, a);
    if (rc != NF_OK) return rc;
    if (B == 0) return fail(NF_EINVAL, "batch statistics of an empty batch are undefined");
    NfDeviceGuard guard;
    if ((rc = guard.enter(h->device)) != NF_OK) return rc;
    return run_batchstats(h, 1, a, moments_out, (hipStream_t)stream, cond);
}

int nf_set_sync(nf_handle *h, nf_allreduce_fn fn, void *user, double *sync_buf, int32_t world_size)
{
    if (!h) return fail(NF_EINVAL, "handle is NULL");
    if (fn && (!sync_buf || world_size < 1)) return fail(NF_EINVAL, "nf_set_sync needs a device buffer of 64 doubles and world_size >= 1");
    std::lock_guard<std::mutex> lock(h->bs_mu);
    h->sync_fn = fn;
    h->sync_user = user;
    h->sync_buf = fn ? sync_buf : nullptr;
    h->sync_world = fn ? world_size : 1;
    return NF_OK;
}

int nf_sums_reduce(const double *wide, double *out3, uint32_t flags, void *stream)
{
    if (!wide || !out3) return fail(NF_EINVAL, "null argument");
    hipError_t e = nf_launch_sums_reduce(wide, out3, (flags & NF_ACCUMULATE) != 0, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "nf_sums_reduce launch");
    return NF_OK;
}

int nf_tile_segments(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int32_t direction,
                     int32_t *out5, int32_t cap)
{
    if (direction != 0 && direction != 1) return fail(NF_EINVAL, "direction must be 0 or 1");
    Built b;
    int rc = build_program(cfg, layers, params, n_params, direction, b);
    if (rc != NF_OK) return rc;
    if (!b.tiled) return 0;
    for (int i = 0; i < (int)b.segs.size() && i < cap && out5; ++i) {
        const Built::TileSeg &g = b.segs[i];
        const int32_t v[5] = {g.op0, g.op1, g.halo, g.ny, g.nx};
        memcpy(out5 + 5 * i, v, sizeof(v));
    }
    return (int)b.segs.size();
}

int nf_tile_plan(int32_t size, int32_t tile, int32_t halo, int32_t *origin, int32_t *core0, int32_t *core1, int32_t cap)
{
    if (size < 1 || tile < 1 || halo < 0 || tile > size) return fail(NF_EINVAL, "bad tile plan (size %d, tile %d, halo %d)", size, tile, halo);
    if (size > tile && tile - 2 * halo < 1) return fail(NF_EINVAL, "a %d-pixel tile has no core with a halo of %d", tile, halo);
    const int n = nf_tile_count(size, tile, halo);
    for (int i = 0; i < n && i < cap; ++i) {
        if (origin) origin[i] = nf_tile_origin(i, size, tile, halo);
        if (core0) core0[i] = nf_tile_core0(i, size, tile, halo);
        if (core1) core1[i] = nf_tile_core1(i, n, size, tile, halo);
    }
    return n;
}

int nf_sample_eps(uint64_t seed, int64_t patch_index_base, int64_t B, int32_t height, int32_t width, float *eps_out, void *stream)
{
    if (B < 0 || height < 1 || width < 1) return fail(NF_EINVAL, "bad shape");
    if (!eps_out || !aligned16(eps_out)) return fail(NF_EINVAL, "eps_out must be a 16-byte aligned device pointer");
    hipError_t e = nf_launch_eps(seed, patch_index_base, B, height * width, eps_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "nf_sample_eps launch");
    return NF_OK;
}

int nf_synth_patches(uint64_t seed, int64_t patch_index_base, int64_t B, int32_t height, int32_t width, float beta1,
                     float beta2, float *y_out, float *x_out, void *stream)
{
    if (B < 0 || height < 1 || width < 1) return fail(NF_EINVAL, "bad shape");
    if (!y_out && !x_out) return fail(NF_EINVAL, "both outputs are NULL");
    hipError_t e = nf_launch_synth(seed, patch_index_base, B, height * width, beta1, beta2, y_out, x_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "nf_synth_patches launch");
    return NF_OK;
}

}  // extern "C"
