// The trainer's matrix-core GEMMs (noise_flow_amd/csrc/nf_train_mm.h) behind a plain-C ABI, for tests/test_gpu_train_mm.py:
// `make -C noise_flow_amd/csrc probe` builds tools/probes/libmm_check.so beside mm_probe.
// The two entry points fill PixArgs / KpixArgs from scalars and DEVICE pointers and call what nf_train_gemm.h calls, with
// Ctx{n_cu, device, mode}: mode 0 = the fp32 kernels, 2 / 3 = "bf16 x 6" on 8 / 4 wavefronts (pix_mode()).  No allocation, no
// synchronisation, no checks of their own: the caller owns every buffer and compares the results.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../noise_flow_amd/csrc/nf_train_mm.h"

static mm::Ctx ctx(int n_cu, int mode)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    return mm::Ctx{n_cu, dev, mode};
}

// C[P][ldc] = pro(A) . Bt^T through mm::mm_pix<APRO, EPI, AV> (the CV 4 / 1 choice stays mm_pix's alignment rule), for the
// combinations nf_train_gemm.h launches with more than 64 output channels.  0: launched; -1: not instantiated; -2: launch failed
extern "C" int mmc_pix(int mode, int apro, int epi, int av, long long P, int N, int K, const float *A, int lda, const float *Bt, int ldb,
                       float *C, int ldc, const float *abias, const float *abn, const float *ebias, const float *ebn, const float *eh, int ldh,
                       const float *ebb, float *stats, int nslot, int n_cu, void *stream)
{
    mm::PixArgs a{};
    a.P = P; a.N = N; a.K = K;
    a.A = A; a.lda = lda; a.Bt = Bt; a.ldb = ldb; a.C = C; a.ldc = ldc;
    a.abias = abias; a.abn = abn;
    a.ebias = ebias; a.ebn = ebn; a.eh = eh; a.ldh = ldh; a.ebb = ebb;
    a.stats = stats; a.nslot = nslot;
    const mm::Ctx cx = ctx(n_cu, mode);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int key = apro * 100 + epi * 10 + av;
    bool ok;
    switch (key) {
    case 14: ok = mm::mm_pix<0, 1, 4>(cx, st, a); break;    // l_1 forward on rows of 20
    case 114: ok = mm::mm_pix<1, 1, 4>(cx, st, a); break;   // l_2 forward
    case 111: ok = mm::mm_pix<1, 1, 1>(cx, st, a); break;
    case 24: ok = mm::mm_pix<0, 2, 4>(cx, st, a); break;    // l_2 transposed
    case 21: ok = mm::mm_pix<0, 2, 1>(cx, st, a); break;
    case 44: ok = mm::mm_pix<0, 4, 4>(cx, st, a); break;    // l_last transposed: the sums, then BN2's backward stored
    case 34: ok = mm::mm_pix<0, 3, 4>(cx, st, a); break;
    default: return -1;
    }
    return ok ? 0 : -2;
}

// part[s][M][N] = sum over the pixels of chunk s of relu(xhat(A + bias))^T . B through mm::mm_kpix_launch<2, 2, 2, 1, 4, 4> (d l_2/W:
// the one launch that turns into k_mm_kpix6 at mode >= 2).  Returns the number of partial products S; -2: launch failed
extern "C" int mmc_kpix(int mode, long long npix, int M, int N, const float *A, int lda, const float *B, int ldb, const float *abias,
                        const float *abn, float *part, long long part_cap, int n_cu, void *stream)
{
    mm::KpixArgs k{};
    k.npix = npix; k.M = M; k.N = N;
    k.A = A; k.lda = lda; k.B = B; k.ldb = ldb;
    k.abias = abias; k.abn = abn;
    k.part = part; k.part_cap = part_cap;
    const int S = mm::mm_kpix_launch<2, 2, 2, 1, 4, 4>(ctx(n_cu, mode), static_cast<hipStream_t>(stream), k);
    return S > 0 ? S : -2;
}
