"""A patch's result does not depend on the batch it sits in — bit for bit, on every kernel path.

Every kernel family is a persistent workgroup that walks several patches through LDS tiles whose zero borders are written once
(and, in the GEMM kernels, through weight slabs, band buffers and partial-sum regions that outlive a patch).  Anything a workgroup
keeps from the patch before — a border pixel, a deferred sum, a stale seam tap — shows as a result that depends on the neighbours
in the batch.  tests/test_split_bf16.py checks this for the two 32x32 width-4 kernels (NF_PATH_SPLIT_BF16, NF_PATH_MFMA4); this
module generalises that test to one small ragged shape on each of the other paths, fp32 and fp16-CNN mode.

Batch size: 2.4 x the number of workgroups the kernel keeps resident, so that workgroups get two and three patches.  The grid of
every launch site is  min(B, multi_processor_count x occ):
  * nf_launch_gemm / gemmb / gemm16 / gemm16b (nf_gemm_common.h, gemm_launch_own): occ = 1, one workgroup per CU;
  * launch_flow_p (nf_kernels.hip), launch_wide_p (nf_wide.hip), launch_wide16 (nf_wide16.hip): occ is what
    hipOccupancyMaxActiveBlocksPerMultiprocessor reports for the kernel, clamped to 1 .. 32.  The test cannot ask for that number,
    so it takes the largest value the hardware allows for the workgroup size the dispatcher picks at the shape (2048 threads per
    CU: 8 workgroups of 256, 4 of 512, 2 of 1024); where registers or LDS hold fewer, workgroups walk more than three patches.
    The slices that straddle the resident count are taken at EVERY multiple of multi_processor_count up to that value, so the true
    count is among them.
"""
import numpy as np
import pytest

from conftest import trained_like_variables
from test_split_bf16 import _mixed_batch

pytestmark = pytest.mark.gpu

ARCH = "sdn5|unc|gain4|unc"

# (path, width, (H, W), cnn_dtype, workgroup size the dispatcher picks at that shape; 0 = the GEMM kernels: one workgroup per CU)
CASES = [
    ("SCALAR", 8, (20, 28), "fp32", 256),          # dispatch_geom: 257 .. 1024 pixels -> 256 threads x 4 pixels
    ("MFMA4", 4, (20, 28), "fp32", 256),
    ("FP16", 4, (64, 64), "fp16", 1024),           # 1025 .. 4096 pixels -> 1024 threads x 4 pixels
    ("WIDE16", 16, (9, 33), "fp32", 512),          # dispatch_wide16: 2 strips of 8 rows x 3 column blocks = 6 wavefronts -> 512
    ("WIDE32", 32, (9, 33), "fp32", 512),          # dispatch_wide: H <= 32 < W -> 512 threads, two tiles per row
    ("WIDE32_FP16", 32, (9, 33), "fp16", 512),
    ("GEMM", 64, (9, 33), "fp32", 0),              # LDS-resident weights
    ("GEMM", 256, (9, 33), "fp32", 0),             # streamed weights
    ("GEMM_FP16", 64, (9, 33), "fp16", 0),
    ("GEMM_FP16", 256, (9, 33), "fp16", 0),
]
IDS = ["%s-w%d-%dx%d" % (c[0].lower(), c[1], c[2][0], c[2][1]) for c in CASES]


def _variables(width, seed):
    v = trained_like_variables(ARCH, width, seed=seed)
    if width > 4:
        for k in v:   # activations of O(1) at every width, as tests/test_gpu_gemm.py::_variables
            if k.endswith("l_2/W") or k.endswith("l_last/W"):
                v[k] = (v[k] * np.float32((4.0 / width) ** 0.5)).astype(np.float32)
    return v


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_patch_result_does_not_depend_on_the_batch(case):
    """Per-patch NLL, sd_z, log-det, latents and eps-supplied samples of the full batch are, bit for bit, what the same patches
    give alone, at the head / tail of smaller batches, in slices that straddle every candidate resident-workgroup count, and in
    the second half of the batch.  No family needed an exemption: every per-patch sum of these kernels is taken in an order that
    depends on the patch's own geometry only."""
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    path, width, (H, W), cnn_dtype, threads = case
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    occ_max = 1 if threads == 0 else min(32, 2048 // threads)
    resident = n_cu * occ_max
    B = int(2.4 * resident)
    m = NoiseFlow([H, W, 4], False, default_hps(arch=ARCH, width=width), variables=_variables(width, seed=9), cnn_dtype=cnn_dtype)
    want = getattr(_lib, "NF_PATH_" + path)
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (case, direction)
    x, y = _mixed_batch(B, seed=31, hw=(H, W))
    eps = np.random.RandomState(5).randn(*x.shape).astype(np.float32)
    eps[np.arange(B) % 5 == 1] = 0.0
    eps[np.arange(B) % 5 == 2] *= 30.0
    cond = m._cond([0.0], [0.0], [800], [2])

    def run(sel):
        xs, ys, es = (torch.as_tensor(a[sel]).cuda() for a in (x, y, eps))
        nll, sd, _, _, _, _ = m._run_nll(xs, ys, cond, False)
        _, _, ld, z, _, _ = m._run_nll(xs, ys, cond, True, _lib.NF_NO_PRIOR)
        smp = m.sample(ys, 1.0, ys, [0.0], [0.0], [800], [2], eps=es)
        return [t.cpu().numpy().copy() for t in (nll, sd, ld, z, smp)]

    full = run(slice(0, B))
    assert all(np.isfinite(a).all() for a in full)
    sels = [slice(0, 1), slice(B - 1, B), slice(B // 2, B)] + [slice(k * n_cu - 3, k * n_cu + 5) for k in range(1, occ_max + 1)]
    for sel in sels:
        for name, a, b in zip(("nll", "sd_z", "log-det", "z", "sample"), run(sel), full):
            assert np.array_equal(a.view(np.uint32), b[sel].view(np.uint32)), (sel, name)
