// The layer vocabulary (NF_LAYER_* of include/noiseflow_hip.h), written once for the evaluator's host code (nf_host.hip) and the
// trainer's host and device code (nf_train.hip and the headers it includes): what a kind IS (class, parameter count, trainable
// ranges, what it reads of nf_cond, its name in error messages), where a coupling's variables sit in its raw block, how nf_cond
// becomes table indices, and how raw parameters become (a, b), a gain scale or a 4x4 matrix.  Functions, tables and constants only:
// no HIP runtime call, nothing that owns memory.  A new kind is one row of kNfLayers plus its formula below.
//
// Every formula is evaluated in double, in ONE order of operations — the evaluator's, which the fold-layout digests and the oracle
// comparisons pin bit for bit on the CPU.  The one exception is k_e_inv4 (nf_train_gemm.h), the batch-statistics evaluator's
// inverse of the matrices k_prep left in float: it multiplies each pivot row by a reciprocal where nf_invert4 divides, and its
// results are pinned bit for bit (tests/test_gpu_trainer_bits.py, bs-*), so its arithmetic stays its own.
//
// oracle/ restates all of this independently and includes none of it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/noiseflow_hip.h"

#define NF_HD __host__ __device__ inline

// ---- constants (each consumer keeps its precision: the evaluator folds in double, the trainer's kernels hold the float literals and
// widen them where they are used)
constexpr int kC = 4;                     // channels of a packed raw patch
constexpr double kBnEps = 1e-4;           // layers.py:378
constexpr float kBnEpsF = 1e-4f;
constexpr float kBnDecayF = 0.1f;         // layers.py:378
constexpr double kLogscaleFactor = 3.0;   // layers.py:653
constexpr float kLogscaleF = 3.0f;
constexpr int kNfIsos = 5, kNfCams = 5;   // ISO 100, 400, 800, 1600, 3200; cameras 0..4 = IP, GP, S6, N6, G4
#define NF_CAM_ERROR "unknown camera id %g (expected 0..4 = IP,GP,S6,N6,G4)"

// ---- the layer table
enum NfClass : uint8_t {
    NF_CLS_NONE,       // no such kind
    NF_CLS_MIX,        // a constant 4x4 matrix per step (Conv2d1x1 in every decomposition, the permutation)
    NF_CLS_SDN,        // z / sqrt(a y + b)
    NF_CLS_COND_GAIN,  // z / scale, the scale a function of nf_cond
    NF_CLS_GAIN,       // z / scale, the scale a variable
    NF_CLS_COUPLING
};

struct NfLayerInfo {
    NfClass cls;
    int16_t count;          // raw parameters (COUPLING: nf_cpl_off(0, w).end)
    int16_t train[2][2];    // up to two trainable ranges [lo, hi) within the block (COUPLING: everything but the BN running moments)
    bool iso, cam, y;       // what it reads: nf_cond.iso, nf_cond.cam, the clean image
    const char *name;       // as the "model has ... but cond is NULL" messages name it
};

constexpr int kNfLayerKinds = 17;
constexpr NfLayerInfo kNfLayers[kNfLayerKinds + 1] = {
    {NF_CLS_NONE, 0, {{0, 0}, {0, 0}}, false, false, false, ""},
    /*  1 CONV1X1      */ {NF_CLS_MIX, 36, {{20, 36}, {0, 0}}, false, false, false, "a Conv2d1x1 layer"},   // P [16], sign_S [4] constant; log_S, L_vec, U_vec
    /*  2 COUPLING     */ {NF_CLS_COUPLING, 0, {{0, 0}, {0, 0}}, false, false, false, "a coupling layer"},
    /*  3 SDN5         */ {NF_CLS_SDN, 23, {{0, 22}, {0, 0}}, true, true, true, "an SDN5 layer"},           // beta1, beta2, gain [5], cam [3][5]; c_i constant
    /*  4 GAIN4        */ {NF_CLS_GAIN, 1, {{0, 1}, {0, 0}}, false, false, false, "a GAIN4 layer"},
    /*  5 SDN4         */ {NF_CLS_SDN, 7, {{0, 7}, {0, 0}}, true, false, true, "an SDN4 layer"},
    /*  6 SDN          */ {NF_CLS_SDN, 2, {{0, 2}, {0, 0}}, false, false, true, "an SDN layer"},
    /*  7 GAIN         */ {NF_CLS_COND_GAIN, 2, {{0, 2}, {0, 0}}, true, false, false, "a GAIN layer"},
    /*  8 SDN1         */ {NF_CLS_SDN, 7, {{0, 7}, {0, 0}}, true, false, true, "an SDN layer with a per-ISO gain table"},
    /*  9 SDN2         */ {NF_CLS_SDN, 7, {{0, 7}, {0, 0}}, true, false, true, "an SDN layer with a per-ISO gain table"},
    /* 10 SDN3         */ {NF_CLS_SDN, 7, {{0, 7}, {0, 0}}, true, false, true, "an SDN layer with a per-ISO gain table"},
    /* 11 SDN6         */ {NF_CLS_SDN, 13, {{0, 12}, {0, 0}}, true, true, true, "an SDN6 layer"},           // beta1, beta2, gain [5], cam [5]; c_i constant
    /* 12 GAIN1        */ {NF_CLS_COND_GAIN, 2, {{0, 2}, {0, 0}}, true, false, false, "a GAIN1 layer"},
    /* 13 GAIN2        */ {NF_CLS_COND_GAIN, 5, {{0, 5}, {0, 0}}, true, false, false, "a per-ISO GAIN layer"},
    /* 14 GAIN3        */ {NF_CLS_COND_GAIN, 5, {{0, 5}, {0, 0}}, true, false, false, "a per-ISO GAIN layer"},
    /* 15 CONV1X1_NONE */ {NF_CLS_MIX, 16, {{0, 16}, {0, 0}}, false, false, false, "a Conv2d1x1 layer"},
    /* 16 CONV1X1_LU2  */ {NF_CLS_MIX, 56, {{16, 32}, {36, 56}}, false, false, false, "a Conv2d1x1 layer"},  // P [16], L [16], sign_S [4], log_S [4], U [16]
    /* 17 PERMUTE      */ {NF_CLS_MIX, 0, {{0, 0}, {0, 0}}, false, false, false, "a permutation"},
};

constexpr bool nf_layer_table_ok()
{
    for (int k = 1; k <= kNfLayerKinds; ++k) {
        const NfLayerInfo &e = kNfLayers[k];
        if (e.cls == NF_CLS_NONE) return false;
        for (int r = 0; r < 2; ++r)
            if (e.train[r][0] < 0 || e.train[r][0] > e.train[r][1] || e.train[r][1] > e.count) return false;
        if (e.train[0][1] > e.train[1][0] && e.train[1][1] > e.train[1][0]) return false;   // two ranges: ascending, disjoint
        if ((e.cls == NF_CLS_SDN) != e.y) return false;
    }
    return true;
}
static_assert(NF_LAYER_PERMUTE == kNfLayerKinds && NF_LAYER_CONV1X1 == 1, "kNfLayers is indexed by NF_LAYER_*");
static_assert(kNfLayers[NF_LAYER_COUPLING].cls == NF_CLS_COUPLING && kNfLayers[NF_LAYER_GAIN4].cls == NF_CLS_GAIN &&
              kNfLayers[NF_LAYER_SDN5].cam && kNfLayers[NF_LAYER_SDN6].cam && kNfLayers[NF_LAYER_CONV1X1_LU2].count == 56, "kNfLayers rows out of order");
static_assert(nf_layer_table_ok(), "every kind has an entry and every trainable range lies inside its block");

// the entry of a kind; class NF_CLS_NONE for a number that is none
inline const NfLayerInfo &nf_layer_info(int type) { return kNfLayers[type >= 1 && type <= kNfLayerKinds ? type : 0]; }

// ---- where a coupling's variables sit in the raw vector: l_1/W [18][w], l_1/b, BN1 mean + var, l_2/W [w][w], l_2/b, BN2 mean + var,
// l_last/W [36][w + 1]; tail3: l_last/b [4], logs [4], rescaling_scale.  The ONE place these formulas are written.
struct CplOff {
    int w1, b1, m1, w2, b2, m2, w3, tail3, end;
};
#define NF_CPL_W3_LEN(w) (36 * ((w) + 1))   // floats of l_last/W (a macro: the kernels that step from l_last/W to tail3 keep their code bit for bit)
NF_HD constexpr CplOff cpl_off(int off, int w)
{
    const int w2 = off + 21 * w, m2 = w2 + w * w + w, w3 = m2 + 2 * w;
    return CplOff{off, off + 18 * w, off + 19 * w, w2, w2 + w * w, m2, w3, w3 + NF_CPL_W3_LEN(w), w3 + NF_CPL_W3_LEN(w) + 9};
}
static_assert(cpl_off(0, 4).end == 301 && cpl_off(0, 1).m1 + 2 <= cpl_off(0, 1).w2 && cpl_off(0, 512).m2 + 1024 <= cpl_off(0, 512).w3,
              "the BN running moments (the holes of the trainable mask: 2 w from m1, 2 w from m2) lie inside the block");

inline int64_t nf_param_count(int32_t type, int32_t w)
{
    const NfLayerInfo &e = nf_layer_info(type);
    if (e.cls == NF_CLS_NONE) return -1;
    if (e.cls != NF_CLS_COUPLING) return e.count;
    if (w <= 0) return -1;
    return 21 * (int64_t)w + (int64_t)w * w + 3 * (int64_t)w + 36 * ((int64_t)w + 1) + 9;   // cpl_off(0, w).end without int overflow
}

// ---- nf_cond -> table indices
struct CondIdx {
    float iso;
    int iso_idx;   // index into a per-ISO table or -1: an ISO outside the table
    int cam_idx;   // 0..4, or -1: no such camera (NF_CAM_ERROR for the kinds that read it)
};
inline CondIdx nf_cond_index(const nf_cond *cond)
{
    constexpr float iso_vals[kNfIsos] = {100.f, 400.f, 800.f, 1600.f, 3200.f};
    CondIdx ci{cond->iso, -1, -1};
    for (int i = 0; i < kNfIsos; ++i)
        if (iso_vals[i] == cond->iso) ci.iso_idx = i;
    for (int i = 0; i < kNfCams; ++i)
        if ((float)i == cond->cam) ci.cam_idx = i;
    return ci;
}
// SDN5 / SDN4 / SDN6: an unknown ISO is an empty one-hot, the gain parameter reads 0 (cond_utils.py:227-229)
NF_HD double nf_onehot_gain(const float *table, CondIdx ci) { return ci.iso_idx >= 0 ? (double)table[ci.iso_idx] : 0.0; }
// the per-ISO tables of the Ex1-Ex3 layers: nested tf.cond whose last branch is the ISO-800 entry (cond_utils.py:69-88)
NF_HD int nf_table_idx(CondIdx ci) { return ci.iso_idx >= 0 ? ci.iso_idx : 2; }

// ---- scalar formulas
NF_HD double nf_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// scale^2 = a y + b of an sdn kind, with what the chain rule of the trainer reads again: the camera factors cp[] and the one-hot
// gain parameter g (SDN5 / SDN6), the gain (SDN1-3) and the two sigmoids (SDN, SDN1-3)
struct NfSdn {
    double a, b, cp[3], g, gain, A0, B0;
};
NF_HD void nf_sdn_eval(int kind, const float *p, CondIdx ci, NfSdn &s)
{
    const double iso = ci.iso;
    if (kind == NF_LAYER_SDN5) {                  // cond_utils.py:205-239
        const double c_i = p[22];
        for (int r = 0; r < 3; ++r) s.cp[r] = exp(c_i * (double)p[7 + r * 5 + ci.cam_idx]);
        s.g = nf_onehot_gain(p + 2, ci);
        s.gain = exp(c_i * s.g * s.cp[2]) * iso;
        s.a = exp(c_i * (double)p[0] * s.cp[0]) / s.gain;
        s.b = exp(c_i * (double)p[1] * s.cp[1]);
    } else if (kind == NF_LAYER_SDN4) {           // cond_utils.py:178-202 (c = 1, no camera)
        s.g = nf_onehot_gain(p + 2, ci);
        s.gain = exp(s.g) * iso;
        s.a = exp((double)p[0]) / s.gain;
        s.b = exp((double)p[1]);
    } else if (kind == NF_LAYER_SDN6) {           // cond_utils.py:242-276: one camera parameter, on the gain exponent only
        const double c_i = p[12];
        s.cp[0] = exp(c_i * (double)p[7 + ci.cam_idx]);
        s.g = nf_onehot_gain(p + 2, ci);
        s.gain = exp(c_i * s.g * s.cp[0]) * iso;
        s.a = exp(c_i * (double)p[0]) / s.gain;
        s.b = exp(c_i * (double)p[1]);
    } else {                                      // SDN (cond_utils.py:41-52), SDN1 (:55-98), SDN2 (:101-138), SDN3 (:141-175)
        s.A0 = nf_sigmoid(p[0]);
        s.B0 = nf_sigmoid(p[1]);
        if (kind == NF_LAYER_SDN) {
            s.a = s.A0;
            s.b = s.B0;
            return;
        }
        s.gain = exp((kind == NF_LAYER_SDN1 ? 1e-2 : 1e-1) * (double)p[2 + nf_table_idx(ci)]) * iso;
        if (kind == NF_LAYER_SDN1) {              // sqrt(b1 y / r_gain + b2)
            s.a = s.A0 / s.gain;
            s.b = s.B0;
        } else if (kind == NF_LAYER_SDN2) {       // sqrt(gain (b1 y / gain + b2))
            s.a = s.gain * (s.A0 / s.gain);
            s.b = s.gain * s.B0;
        } else {                                  // gain sqrt(b1 y / gain + b2)
            s.a = s.gain * s.gain * (s.A0 / s.gain);
            s.b = s.gain * s.gain * s.B0;
        }
    }
}

// scale of a gain kind and K, the number of log(scale) terms its log-det holds (cond_utils.py:319-440 and the layers: GainEx4 /
// GainEx2 write the full H*W*C sum, Gain / GainEx1 / GainEx3 -log(scale) once per patch, e.g. AffineCouplingGain.py:113-127)
NF_HD void nf_gain_eval(int kind, const float *p, CondIdx ci, int HW, double &sv, double &K)
{
    const double iso = ci.iso;
    K = 1.0;
    if (kind == NF_LAYER_GAIN4) { sv = p[0]; K = 4.0 * HW; }
    else if (kind == NF_LAYER_GAIN) sv = nf_sigmoid(p[0]) * iso + nf_sigmoid(p[1]);
    else if (kind == NF_LAYER_GAIN1) sv = exp(1e-5 * (double)p[0]) * iso + exp(1e-5 * (double)p[1]);
    else if (kind == NF_LAYER_GAIN2) { sv = exp(1e-1 * (double)p[nf_table_idx(ci)]) * iso; K = 4.0 * HW; }
    else sv = exp(1e-5 * (double)p[nf_table_idx(ci)]);
}

// ---- the 4x4 matrix of a Conv2d1x1
struct Mat4 {
    double m[4][4];
};

NF_HD Mat4 nf_matmul(const Mat4 &a, const Mat4 &b)
{
    Mat4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}

// vector element k -> matrix entry (row, column) of tfdist.fill_triangular padded to a strict 4x4 triangle (matrix_param.py:31-56):
// lower [[v3,0,0],[v5,v4,0],[v2,v1,v0]] under a zero row, upper [[v0,v1,v2],[0,v4,v5],[0,0,v3]] right of a zero column.  X-lists, so
// that every use (the matrices here, the trainer's gradient of L_vec / U_vec) indexes with constants.
#define NF_TRI_LOWER(X) X(0, 3, 2) X(1, 3, 1) X(2, 3, 0) X(3, 1, 0) X(4, 2, 1) X(5, 2, 0)
#define NF_TRI_UPPER(X) X(0, 0, 1) X(1, 0, 2) X(2, 0, 3) X(3, 2, 3) X(4, 1, 2) X(5, 1, 3)

// P, L, U and log|det| of decomp = LU (matrix_param.py:100-140): P [16], sign_S [4], log_S [4], L_vec [6], U_vec [6]
NF_HD double nf_plu_matrices(const float *p, Mat4 &Pm, Mat4 &L, Mat4 &U)
{
    const float *sign_s = p + 16, *log_s = p + 20, *lv = p + 24, *uv = p + 30;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            Pm.m[i][j] = p[i * 4 + j];
            L.m[i][j] = i == j ? 1.0 : 0.0;
            U.m[i][j] = 0.0;
        }
#define NF_X(k, r, c) L.m[r][c] = lv[k];
    NF_TRI_LOWER(NF_X)
#undef NF_X
#define NF_X(k, r, c) U.m[r][c] = uv[k];
    NF_TRI_UPPER(NF_X)
#undef NF_X
    double lad = 0.0;
    for (int i = 0; i < 4; ++i) {
        U.m[i][i] = (double)sign_s[i] * exp((double)log_s[i]);
        lad += (double)log_s[i];
    }
    return lad;
}

// ... of decomp = LU2 (matrix_param.py:143-188): P [16], L [16], sign_S [4], log_S [4], U [16]; the full-matrix L / U variables
// masked to their strict triangles
NF_HD double nf_lu2_matrices(const float *p, Mat4 &Pm, Mat4 &L, Mat4 &U)
{
    const float *Lf = p + 16, *sign_s = p + 32, *log_s = p + 36, *Uf = p + 40;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            Pm.m[i][j] = p[i * 4 + j];
            L.m[i][j] = j < i ? (double)Lf[i * 4 + j] : (i == j ? 1.0 : 0.0);
            U.m[i][j] = j > i ? (double)Uf[i * 4 + j] : (i == j ? (double)sign_s[i] * exp((double)log_s[i]) : 0.0);
        }
    double lad = 0.0;
    for (int i = 0; i < 4; ++i) lad += (double)log_s[i];           // :187
    return lad;
}

// A = P (L U), row-major into A16 (the evaluator's Mat4 in double, the trainer's float buffer: the sums are double either way)
template <class T>
NF_HD void nf_plu_product(const Mat4 &Pm, const Mat4 &L, const Mat4 &U, T *A16)
{
    const Mat4 LU = nf_matmul(L, U);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += Pm.m[i][k] * LU.m[k][j];
            A16[i * 4 + j] = (T)s;
        }
}

// the matrix of decomp = NONE (matrix_param.py:23-29: the variable) and of the permutation (channels reversed, noise_flow_model.py:80-84)
NF_HD Mat4 nf_mat_of(const float *p)
{
    Mat4 A;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) A.m[i][j] = p[i * 4 + j];
    return A;
}
template <class T>
NF_HD void nf_mat_reverse(T *A16)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) A16[i * 4 + j] = (i + j == 3) ? (T)1 : (T)0;
}

// General 4x4 inverse + log|det| by Gauss-Jordan with partial pivoting, in double (tf.matrix_inverse / tf.linalg.slogdet of
// matrix_param.py:26-27, :177-179).  false = a pivot was zero: the matrix is singular and `inv` is not written.
NF_HD bool nf_invert4(const Mat4 &M, Mat4 &inv, double &log_abs_det)
{
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            a[i][j] = M.m[i][j];
            a[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    log_abs_det = 0.0;
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (!(fabs(a[piv][c]) > 0.0)) return false;
        if (piv != c)
            for (int j = 0; j < 8; ++j) {
                const double t = a[piv][j];
                a[piv][j] = a[c][j];
                a[c][j] = t;
            }
        const double d = a[c][c];
        log_abs_det += log(fabs(d));
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv.m[i][j] = a[i][4 + j];
    return true;
}
