"""Which of its three routes a batch-statistics call takes (csrc/nf_host.hip: bs_route — the width-4 matrix-core schedule, the
scalar-weight schedule, or the layer-by-layer evaluator on the trainer's kernels), as nf_batchstats_route reports it, over widths x
patch shapes x the per-call switches NF_BS_WIDE / NF_TRAIN_PR.

The expected values restate the conditions of the code before the decision had one place (commit f36931b), and every row was
confirmed against that build by the kernels it launched (profiles/r17_batchstats_host_launches.txt: tools/batchstats_launches.py
runs these rows too).  Only nf_create / nf_batchstats_route / nf_destroy are called: no kernel is launched.  NF_KERNEL=valu is read
once per process, so those rows are computed in one fresh child process.
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MFMA4, SCALAR, TRAINER = 0, 1, 2      # _lib.NF_BS_ROUTE_*
SWITCHES = ("NF_BS_WIDE", "NF_TRAIN_PR")

# (coupling width, H, W, switches of the call, NF_KERNEL mode of the process, route)
ROWS = [
    (4, 32, 32, {}, None, MFMA4),
    (4, 32, 32, {"NF_BS_WIDE": "1"}, None, TRAINER),
    (4, 128, 128, {}, None, MFMA4),                     # tiled: the matrix-core schedule takes every size
    (4, 32, 32, {}, "valu", SCALAR),
    (4, 128, 128, {}, "valu", TRAINER),                 # tiled, and no matrix-core schedule
    (8, 24, 40, {}, None, SCALAR),
    (8, 64, 64, {}, None, TRAINER),                     # 174 KiB of LDS
    (5, 8, 8, {}, None, SCALAR),                        # padded to 8
    (16, 16, 16, {}, None, SCALAR),
    (16, 48, 64, {}, None, TRAINER),
    (32, 20, 12, {}, None, SCALAR),
    (32, 32, 32, {}, None, TRAINER),                    # the patch-resident stages
    (32, 32, 32, {"NF_TRAIN_PR": "0"}, None, SCALAR),
    (32, 64, 64, {}, None, TRAINER),
    (64, 8, 8, {}, None, TRAINER),
    (8, 128, 128, {}, None, TRAINER),
]
ARCH = "unc|gain4|unc"


def row_key(row):
    w, H, W, env, kernel, _ = row
    return "w%d;%dx%d;%s;%s" % (w, H, W, ",".join("%s=%s" % kv for kv in sorted(env.items())), kernel or "")


def make_model(width, H, W, cnn_dtype=None):
    from conftest import trained_like_variables
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([H, W, 4], True, default_hps(arch=ARCH, width=width), variables=trained_like_variables(ARCH, width, seed=width),
                     cnn_dtype=cnn_dtype)


def compute_rows(kernel):
    """{row key: route} of the rows of THIS process's NF_KERNEL mode."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    keep = {k: os.environ.pop(k, None) for k in SWITCHES}
    out = {}
    try:
        for row in ROWS:
            w, H, W, env, k, _ = row
            if k != kernel:
                continue
            m = make_model(w, H, W)
            os.environ.update(env)
            try:
                out[row_key(row)] = int(lib.nf_batchstats_route(m._flow.ptr))
            finally:
                for name in env:
                    del os.environ[name]
    finally:
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    return out


def _expected(kernel):
    return {row_key(r): r[5] for r in ROWS if r[4] == kernel}


@pytest.mark.gpu
def test_route_of_every_row():
    assert "NF_KERNEL" not in os.environ, "these rows are the default (matrix-core) mode"
    got = compute_rows(None)
    assert got == _expected(None)
    assert set(got.values()) == {MFMA4, SCALAR, TRAINER}


@pytest.mark.gpu
def test_route_of_every_row_under_nf_kernel_valu():
    env = dict(os.environ, NF_KERNEL="valu")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child exited with %d\n%s%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert json.loads(p.stdout.strip().splitlines()[-1]) == _expected("valu")


@pytest.mark.gpu
def test_fp16_cnn_handle_is_refused_by_the_call_and_reported_as_einval():
    """The call's refusal stays NF_EINVAL "fp32 only"; the diagnostic returns the same code where the call would refuse."""
    from conftest import make_inputs
    from noise_flow_amd import _lib
    m = make_model(4, 32, 32, cnn_dtype="fp16")
    assert m._flow.lib.nf_batchstats_route(m._flow.ptr) == _lib.NF_EINVAL
    assert m._flow.lib.nf_batchstats_route(None) == _lib.NF_EINVAL
    x, y = make_inputs(2, 32, 32, seed=1)
    with pytest.raises(_lib.NoiseFlowLibError) as e:
        m._loss(x, y, [0.0], [0.0], [400], [1])
    assert "error %d:" % _lib.NF_EINVAL in str(e.value) and "fp32 only" in str(e.value)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    if sys.argv[1:2] == ["--rows"]:
        print(json.dumps(compute_rows(os.environ.get("NF_KERNEL") or None), sort_keys=True))
    else:
        sys.exit(__doc__)
