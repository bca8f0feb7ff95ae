"""The host side of the batch-statistics calls (csrc/nf_host.hip: bs_route, the plan and the one schedule walker behind
nf_nll_batchstats / nf_sample_batchstats) decides launches, operands and their order on the stream — never arithmetic.  A rewrite
of it that keeps every launch and operand must give the bits of the code before it: tests/golden/batchstats_host_bits.npz was
recorded with tools/make_golden_batchstats_bits.py on an MI355X from the build of commit f36931b, the last one with the two
hand-written schedules.  array_equal on the uint32 views, no tolerance; every case also asserts its route (nf_batchstats_route).

Per case: per-patch NLL, the latent from inverse(), a sample from supplied eps, a sample drawn in-kernel from seed= (NF_K_PHILOX_IN
has to be stripped behind the first launch: every later launch reads a resident tensor), and the running moments the four calls
leave.  sd_z and the sums are added with atomics in arrival order and are not recorded.  Long vectors are kept as in
tests/test_gpu_trainer_bits.py (_keep: ends and two sums of the bit patterns per patch).

Which bits are reproducible: the statistics are fp64 atomics into slot `blockIdx & 63`.  The matrix-core kernel adds once per
workgroup and patch after a fixed-order sum, the scalar-weight kernel once per wavefront; with at most 64 workgroups — and, on the
scalar-weight kernel, patches of at most 64 pixels = one wavefront — no slot receives two additions and the bits are fixed BY
CONSTRUCTION (the cases without `generic`).  The `generic` cases have several wavefronts per slot; their bits are fixed only if every
fp64 sum of the wavefront totals is exact, which holds for generic data but not by construction: such a case is in the table only
because the two recordings from the parent build, in two processes, agreed in every bit (the recording tool drops one that does not
and says so; none was dropped)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import FULL_ARCH
from test_gpu_trainer_bits import _env, _keep, _seed, _variables, differing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batchstats_host_bits.npz")
ROUTE_MFMA4, ROUTE_SCALAR, ROUTE_TRAINER = 0, 1, 2      # _lib.NF_BS_ROUTE_*
FOLD, G3 = "sdn5|unc|unc|gain4|unc", "unc|gain4|unc"
HALO = 3                                                # the one halo of a tiled batch-statistics call (csrc/nf_host.hip)


def _c(cid, arch, width, hw, B, route, env=None, kernel=None, generic=False):
    """kernel: the NF_KERNEL mode of the process (read once per process: such a case runs in a child)."""
    return dict(id=cid, arch=arch, width=width, hw=hw, B=B, route=route, env=dict(env or {}), kernel=kernel, generic=generic)


CASES = [
    # ---- width 4 on the matrix-core kernel
    _c("mc-1cpl-8x8", "unc", 4, (8, 8), 3, ROUTE_MFMA4),                            # one coupling: no resident tensor, the final launch is the whole program
    _c("mc-2cpl-10x12", "unc|unc", 4, (10, 12), 3, ROUTE_MFMA4),                    # carry out, never added
    _c("mc-fold-16x24", FOLD, 4, (16, 24), 5, ROUTE_MFMA4),                         # carry added; layers between and behind
    _c("mc-ends-in-gain-10x12", "unc|unc|gain4", 4, (10, 12), 3, ROUTE_MFMA4),
    _c("mc-full-32x32", FULL_ARCH, 4, (32, 32), 6, ROUTE_MFMA4),                    # the shipped architecture
    _c("mc-g3-64x64", G3, 4, (64, 64), 2, ROUTE_MFMA4),
    _c("mc-g3-72x96-tiled", G3, 4, (72, 96), 2, ROUTE_MFMA4),                       # tiles + the tile-combine kernel
    # ---- the scalar-weight kernel, one wavefront per patch
    _c("sc-w8-1cpl", "unc", 8, (8, 8), 5, ROUTE_SCALAR),
    _c("sc-w8-2cpl", "unc|unc", 8, (8, 8), 5, ROUTE_SCALAR),
    _c("sc-w8-3cpl", "unc|unc|unc", 8, (8, 8), 5, ROUTE_SCALAR),
    _c("sc-w16-g3", G3, 16, (8, 8), 4, ROUTE_SCALAR),
    _c("sc-w32-u3", "unc|unc|unc", 32, (8, 8), 3, ROUTE_SCALAR),
    _c("sc-w5-g3", G3, 5, (8, 8), 4, ROUTE_SCALAR),                                 # caller rows of 5 inside kernel rows of 8
    _c("sc-w4-fold-valu", FOLD, 4, (8, 8), 5, ROUTE_SCALAR, kernel="valu"),
    # ---- the scalar-weight kernel, several wavefronts per slot (module docstring: `generic`)
    _c("sc-w8-24x40", "unc|unc", 8, (24, 40), 6, ROUTE_SCALAR, generic=True),       # several pixels per lane: stats_flush
    _c("sc-w16-16x16", G3, 16, (16, 16), 9, ROUTE_SCALAR, generic=True),
    _c("sc-w32-32x32-pr0", "unc|unc", 32, (32, 32), 3, ROUTE_SCALAR, {"NF_TRAIN_PR": "0"}, generic=True),
]
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def _run(case, res):
    from noise_flow_amd import _lib
    from conftest import make_inputs
    from test_gpu_batchstats import _model
    H, W = case["hw"]
    B = case["B"]
    x, y = make_inputs(B, H, W, seed=_seed(case) + 20)
    m = _model(case["arch"], _variables(case), (H, W, 4), case["width"])
    lib = _lib.load()
    route = int(lib.nf_batchstats_route(m._flow.ptr)) if hasattr(lib, "nf_batchstats_route") else None   # (the parent build has none)
    nll, _ = m._loss(x, y, [0.0], [0.0], [400], [1])
    z, _ = m.inverse(x, None, y, [0.0], [0.0], [400], [1])
    eps = np.random.RandomState(_seed(case)).randn(B, H, W, 4).astype(np.float32)
    xs = m.sample(y, 0.6, y, [0.0], [0.0], [400], [1], eps=eps)
    xp = m.sample(y, 0.6, y, [0.0], [0.0], [400], [1], seed=77)
    per_patch = [(i * H * W * 4, (i + 1) * H * W * 4) for i in range(B)]
    res["nll"] = np.asarray(nll, np.float32).reshape(-1)
    _keep(res, "z", z, per_patch)
    _keep(res, "sample", xs, per_patch)
    _keep(res, "sample_seed", xp, per_patch)
    mv = m.variables      # the running moments after two NLL-direction calls and two sampling calls
    res["moments"] = np.concatenate([np.asarray(mv[k], np.float32).reshape(-1) for k in sorted(mv) if "bn_nvp_conv" in k])
    return route


def case_outputs(case):
    """({"<case id>__<name>": array}, route or None) of one case from the library that is loaded."""
    if (case["kernel"] or None) != (os.environ.get("NF_KERNEL") or None):
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "case.npz")
            env = dict(os.environ)
            env.pop("NF_KERNEL", None)
            if case["kernel"]:
                env["NF_KERNEL"] = case["kernel"]
            subprocess.run([sys.executable, os.path.abspath(__file__), case["id"], out], check=True, env=env, timeout=300)
            with np.load(out) as f:
                res = {k: f[k] for k in f.files}
            route = res.pop("route", None)
            return res, None if route is None else int(route)
    res = {}
    with _env(case["env"]):
        route = _run(case, res)
    for name, a in res.items():
        assert a.dtype in (np.float32, np.uint64) and (a.dtype == np.uint64 or np.isfinite(a).all()), (case["id"], name)
    return {"%s__%s" % (case["id"], name): a for name, a in res.items()}, route


def n_tiles(case):
    """Workgroups per patch: the tiles of an image beyond 64x64 under the call's one halo, from nf_tile_plan."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    H, W = case["hw"]
    if H <= 64 and W <= 64:
        return 1
    return lib.nf_tile_plan(H, min(H, 64), HALO, None, None, None, 0) * lib.nf_tile_plan(W, min(W, 64), HALO, None, None, None, 0)


def test_the_cases_cover_the_regimes_they_name():
    """No GPU: the facts the case table relies on, restated from csrc/nf_host.hip and the kernels' statistics epilogues."""
    n_cpl = lambda c: c["arch"].split("|").count("unc")
    for c in CASES:
        H, W = c["hw"]
        tiles = n_tiles(c)
        if c["route"] == ROUTE_MFMA4:
            assert c["width"] == 4 and c["kernel"] is None and not c["generic"]
            assert c["B"] * tiles <= 64, c["id"]                   # one addition per slot
        else:
            assert c["route"] == ROUTE_SCALAR and tiles == 1
            assert (c["width"] == 4) == (c["kernel"] == "valu")   # width 4 reaches the scalar-weight kernel only without the matrix core
            assert c["B"] <= 64
            assert c["generic"] == (H * W > 64), c["id"]           # by construction: one wavefront per patch
            assert c["generic"] or c["B"] <= 5
            # both LDS tiles of the patch fit (scalar_fits), at the padded width
            pw = 4 if c["width"] <= 4 else 8 if c["width"] <= 8 else 16 if c["width"] <= 16 else 32
            tile_px = ((H + 2) * (W + 2) + 1) & ~1
            assert 4 * (tile_px * (2 + pw) + 64) <= 160 * 1024 and not (pw >= 32 and H * W > 1024)
    by = {c["id"]: c for c in CASES}
    assert n_tiles(by["mc-g3-72x96-tiled"]) > 1 and all(n_tiles(c) == 1 for c in CASES if c["id"] != "mc-g3-72x96-tiled")
    assert [n_cpl(by[i]) for i in ("mc-1cpl-8x8", "mc-2cpl-10x12", "mc-fold-16x24", "mc-full-32x32")] == [1, 2, 3, 8]
    assert [n_cpl(by[i]) for i in ("sc-w8-1cpl", "sc-w8-2cpl", "sc-w8-3cpl", "sc-w4-fold-valu")] == [1, 2, 3, 3]
    assert by["mc-ends-in-gain-10x12"]["arch"].endswith("gain4") and by["mc-fold-16x24"]["arch"].startswith("sdn5")
    assert by["sc-w32-32x32-pr0"]["env"] == {"NF_TRAIN_PR": "0"}     # without it: the trainer route


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_batchstats_gives_the_bits_of_the_host_code_before_the_reorganisation(case):
    prefix = case["id"] + "__"
    with np.load(GOLDEN) as f:
        want = {k: f[k] for k in f.files if k.startswith(prefix)}
    assert want, "no golden arrays for %s" % case["id"]
    got, route = case_outputs(case)
    assert route == case["route"], "nf_batchstats_route says %r" % (route,)
    bad = differing(got, want)
    assert not bad, bad


if __name__ == "__main__":      # the child of a case in another NF_KERNEL mode: python test_gpu_batchstats_bits.py <case id> <out.npz>
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if os.environ.get("NF_TOOL_LIB"):      # (tools/make_golden_batchstats_bits.py records from another build)
        from noise_flow_amd import _lib as _l
        _l.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])
    _res, _route = case_outputs(CASES[CASE_IDS.index(sys.argv[1])])
    if _route is not None:
        _res["route"] = np.asarray(_route, np.int64)
    np.savez(sys.argv[2], **_res)
