// Host-side helpers shared by the translation units of libnoiseflow_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/noiseflow_hip.h"

// record a thread-local error message (returned by nf_last_error) and hand back `code`
int nf_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int nf_fail_hip(hipError_t e, const char *what);

// "switch to the handle's device, switch back" around every entry point that touches the device
struct NfDeviceGuard {
    int prev = -1;
    bool changed = false;
    int enter(int dev)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return nf_fail_hip(e, "hipGetDevice");
        if (prev != dev) {
            if ((e = hipSetDevice(dev)) != hipSuccess) return nf_fail_hip(e, "hipSetDevice");
            changed = true;
        }
        return NF_OK;
    }
    ~NfDeviceGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

// geometry / device of a handle (nf_hostfed.hip sizes its staging from them)
struct nf_handle;
int nf_handle_geometry(const nf_handle *h, int32_t *H, int32_t *W, int32_t *device);
// frees the handle's host-fed pipeline, if one was created (nf_destroy)
void nf_hostpipe_release(nf_handle *h);

// Evaluation under batch statistics at the coupling widths / patch sizes the fused kernels' statistics passes do not take
// (nf_train.hip: a trimmed trainer whose couplings run on the matrix-core GEMMs of nf_train_mm.h); owned by the handle's
// batch-statistics state, freed with nf_trainer_destroy
struct nf_bs_wide_args {
    int direction;             // 0: NLL, 1: sampling
    const float *in;           // x (NLL) / epsilon (sampling; NULL: the in-kernel Philox draw keyed by seed, patch_base + b, pixel)
    const float *y;
    int64_t B;
    const nf_cond *cond;
    uint64_t seed;
    int64_t patch_base;
    float in_scale;            // sampling: the temperature; NLL: 1
    float *out;                // z_out (may be NULL) / x_out
    float *nll_out, *sd_out, *ld_out;
    double *sums;              // DEVICE double[3], accumulated into
    bool prior;
    float *moments_out;        // HOST [n_couplings][4][w] or NULL
    nf_allreduce_fn sync_fn;
    void *sync_user;
    double *sync_buf;
    int sync_world;
};
int nf_bs_wide_create(const nf_config *cfg, const nf_layer_desc *layers, const float *params, size_t n_params, int64_t max_batch,
                      nf_trainer **out);
int64_t nf_bs_wide_capacity(const nf_trainer *t);
int nf_bs_wide_run(nf_trainer *t, const nf_bs_wide_args &a, hipStream_t st);

// The gradient kernels' launchers (nf_grad.hip, nf_grad_wide.hip, nf_grad_gemm.hip, nf_sample_grad.hip, nf_sample_grad_wide.hip,
// nf_sample_grad_gemm.hip), called by nf_host.hip, which has
// checked the supported set (grad_support, sample_vjp_support).  `tiled`: one segment of a tiled call (nf_device.h, "gradient tiles") —
// `prog` = the segment's ops, a.H x a.W = the tile, a.B = images x tiles, n_cpl = the couplings of the call's largest segment (what
// a.gate_words / the scratch were sized by); otherwise whole patches and n_cpl = the program's couplings.
// GEMM: `scratch` holds nf_grad_gemm_groups(a.B, n_cu) x nfgg_gate_halves(H W, width, n_cpl) uint16 of gate records.
struct NfProgram;
struct NfGradLaunch;
struct NfSampleGradLaunch;
struct NfSampleGradTileLaunch;
hipError_t nf_launch_grad(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, hipStream_t stream);
hipError_t nf_launch_grad_wide(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, hipStream_t stream);
hipError_t nf_launch_grad_gemm(const NfProgram &prog, const NfGradLaunch &a, bool tiled, int n_cpl, int n_cu, void *scratch, size_t scratch_bytes,
                               hipStream_t stream);
int nf_grad_gemm_groups(int64_t B, int n_cu);   // the persistent grid of the GEMM kernel: one workgroup per CU, never more than patches
hipError_t nf_launch_sample_grad(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, hipStream_t stream);
// NF_SVJP_PATH_TILED: one segment of a tiled call, as `tiled` above (a.n_cpl = the segment's own couplings)
hipError_t nf_launch_sample_grad_tiled(const NfProgram &prog, const NfSampleGradTileLaunch &a, int n_cpl, int n_cu, hipStream_t stream);
// gtemp of a tiled nf_sample_vjp: out[b] = the nt tile sums of image b at part + b nt, added in tile order
hipError_t nf_launch_tile_sum(const float *part, int nt, int64_t B, float *out, hipStream_t stream);
// NF_SVJP_PATH_WIDE32: programs over the NFGW_* block, a.gate_words = nfgw_tpw(a.H) x a.n_cpl
hipError_t nf_launch_sample_grad_wide(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, hipStream_t stream);
// NF_SVJP_PATH_GEMM (nf_sample_grad_gemm.hip): programs over the NFGG_* block; `scratch` as nf_launch_grad_gemm's, sized by a.n_cpl
hipError_t nf_launch_sample_grad_gemm(const NfProgram &prog, const NfSampleGradLaunch &a, int n_cu, void *scratch, size_t scratch_bytes,
                                      hipStream_t stream);
