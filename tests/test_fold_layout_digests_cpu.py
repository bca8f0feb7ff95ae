"""Bit identity of everything the host program builder (csrc/nf_host.hip: build_program) produces, without a GPU.

tests/golden/fold_layout_digests.json holds, for a grid of models x patch shapes x nf_config.flags x environment switches, both
directions and all nine kernel paths, a SHA-256 over what nf_fold_layout returns — the (type, offset) pairs of the program, the
layout's width and the bytes of its parameter block — or, where the call returns no block, its return code; and per case the
digest of nf_fold_params' block, its ld_const (exact, as a hex float) and the segments of nf_tile_segments.  The fixture was
recorded by tools/make_golden_fold_digests.py from the build of the commit BEFORE the builder's op loops and re-layout headers
were merged (the file names it) and never from the code under test: a rewrite of the builder that moves one float, reorders one
op or drops one layout shows here.

The models are built from nf_layer_param_count and numpy's uniform generator alone (exact integer arithmetic -> float32), so the
inputs are the same bits on every machine.
"""
import ctypes as C
import hashlib
import json
import os
import time

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_layout_digests.json")
N_PATHS = 9
ENV_SWITCHES = ("NF_GEMM", "NF_GEMM16", "NF_H16", "NF_TILE_SEGMENTS")

WIDTHS = (3, 4, 6, 8, 12, 16, 24, 32, 40, 64, 96, 200, 512)
SHAPES = ((5, 9), (16, 16), (32, 32), (50, 50), (64, 64), (96, 80), (128, 128))
MAIN = ("sdn5|unc|gain4|unc|gain|unc", 1, "LU")
OTHERS = (("unc|gain4|unc", 0, "LU"), ("unc|unc", 2, "LU"), ("sdn|unc|unc", 1, "LU2"), ("unc|gain4|unc", 1, "NONE"))
PADDED = {3: 4, 6: 8, 12: 16, 24: 32, 40: 64, 96: 128, 200: 256}   # width of the variables -> of the narrowest layout that holds it


def _flags():
    from noise_flow_amd import _lib
    return (0, _lib.NF_CFG_FP16_CNN, _lib.NF_CFG_EXACT_FP32)


def grid():
    """(arch, flow_permutation, decomp, width, H, W, flags, env) — env = "" or "NAME=value".  The main architecture takes the
    widths x shapes x flags product, except that the two widest models (whose blocks are megabytes) take three shapes and one,
    and that NF_CFG_EXACT_FP32 — which only decides between two width-4 layouts — goes to the widths up to 8 and to one GEMM
    width; the other architectures and the environment switches take the cases that reach them."""
    f0, f16, fex = _flags()
    out = []
    for w in WIDTHS:
        for hw in SHAPES:
            if (w == 200 and hw not in ((5, 9), (64, 64), (128, 128))) or (w == 512 and hw != (32, 32)):
                continue
            for fl in (f0, f16, fex):
                if fl == fex and w > 8 and w != 40:
                    continue
                out.append(MAIN + (w,) + hw + (fl, ""))
    for a in OTHERS:
        for w in (4, 8, 40):
            for hw in ((32, 32), (96, 80)):
                for fl in (f0, f16):
                    out.append(a + (w,) + hw + (fl, ""))
    for w in (40, 96):
        for hw in ((16, 16), (32, 32), (64, 64), (128, 128)):
            out.append(MAIN + (w,) + hw + (f0, "NF_GEMM=a"))
            out.append(MAIN + (w,) + hw + (f16, "NF_GEMM16=a"))
    for w in (3, 4):
        for hw in ((5, 9), (32, 32), (64, 64), (128, 128)):
            out.append(MAIN + (w,) + hw + (f16, "NF_H16=4x4"))
    return out


_MODELS = {}


def model(arch, flow_permutation, decomp, width):
    """(descs, flat raw parameters) of an architecture at a coupling width, built once: every layer's parameters uniform in
    (-0.4, 0.4), then what the folding needs — permutation matrices, signs, positive variances and gains."""
    key = (arch, flow_permutation, decomp, width)
    if key in _MODELS:
        return _MODELS[key]
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers = params.parse_arch(arch, flow_permutation, decomp)
    rng = np.random.RandomState(7919 * width + 31 * flow_permutation + len(arch) + len(decomp))
    perm = np.eye(4, dtype=np.float64)[[2, 0, 3, 1]].reshape(-1)
    chunks, offs, pos = [], [], 0
    for L in layers:
        w = width if L.kind == "coupling" else 0
        n = lib.nf_layer_param_count(L.nf_type, w)
        assert n >= 0
        p = (rng.rand(n) - 0.5) * 0.8
        if L.kind in ("conv1x1", "conv1x1_lu2"):
            p[0:16] = perm
            s = 16 if L.kind == "conv1x1" else 32
            p[s:s + 4] = (1.0, -1.0, 1.0, -1.0)
        elif L.kind == "conv1x1_none":
            p += 2.0 * np.eye(4).reshape(-1)
        elif L.kind == "coupling":
            v1, v2 = 20 * w, 23 * w + w * w
            p[v1:v1 + w] = 0.5 + rng.rand(w)
            p[v2:v2 + w] = 0.5 + rng.rand(w)
            p[n - 5:n - 1] *= 0.25          # l_last/logs
            p[n - 1] = 0.3 + 0.6 * rng.rand()   # rescaling_scale
        elif L.kind == "sdn5":
            p[22] = 1.0
        elif L.kind == "gain4":
            p[0] = 1.3
        chunks.append(p.astype(np.float32))
        offs.append(pos)
        pos += n
    flat = np.ascontiguousarray(np.concatenate(chunks), np.float32)
    descs = (_lib.nf_layer_desc * len(layers))()
    for d, L, off in zip(descs, layers, offs):
        d.type, d.width, d.param_offset = L.nf_type, (width if L.kind == "coupling" else 0), off
    _MODELS[key] = (descs, flat)
    return _MODELS[key]


def case_key(case):
    arch, fp, decomp, w, H, W, fl, env = case
    return "%s;p%d;%s;w%d;%dx%d;f%d;%s" % (arch, fp, decomp, w, H, W, fl, env)


def compute_case(lib, case):
    """{"d0": ..., "d1": ...}: per direction the nine nf_fold_layout answers (hex digest, or the return code where there is no
    block), nf_fold_params' digest and ld_const, and nf_tile_segments' rows."""
    from noise_flow_amd import _lib
    arch, fp, decomp, w, H, W, fl, env = case
    descs, flat = model(arch, fp, decomp, w)
    cfg = _lib.nf_config(H, W, 4, len(descs), -1, fl)
    fptr = flat.ctypes.data_as(C.POINTER(C.c_float))
    ops = (C.c_int32 * 256)()
    rec = {}
    for direction in (0, 1):
        paths = []
        for path in range(N_PATHS):
            n_ops, lw, nf = C.c_int32(), C.c_int32(), C.c_size_t()
            head = (C.byref(cfg), descs, fptr, flat.size, direction, path, ops, 128, C.byref(n_ops), C.byref(lw))
            rc = lib.nf_fold_layout(*head, None, 0, C.byref(nf))
            if rc != 0:
                paths.append(rc)
                continue
            blk = np.empty(nf.value, np.float32)
            rc = lib.nf_fold_layout(*head, blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(nf))
            assert rc == 0 and nf.value == blk.size
            h = hashlib.sha256()
            h.update(np.asarray(ops[:2 * n_ops.value], np.int32).tobytes())
            h.update(np.int32(lw.value).tobytes())
            h.update(blk.tobytes())
            paths.append(h.hexdigest())
        n_ops, nf, ld = C.c_int32(), C.c_size_t(), C.c_double()
        head = (C.byref(cfg), descs, fptr, flat.size, direction, ops, 128, C.byref(n_ops))
        rc = lib.nf_fold_params(*head, None, 0, C.byref(nf), C.byref(ld))
        if rc != 0:
            fold, ldc = rc, None
        else:
            blk = np.empty(nf.value, np.float32)
            assert lib.nf_fold_params(*head, blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(nf), C.byref(ld)) == 0
            h = hashlib.sha256()
            h.update(np.asarray(ops[:2 * n_ops.value], np.int32).tobytes())
            h.update(blk.tobytes())
            fold, ldc = h.hexdigest(), float(ld.value).hex()
        seg = (C.c_int32 * 40)()
        ns = lib.nf_tile_segments(C.byref(cfg), descs, fptr, flat.size, direction, seg, 8)
        rec["d%d" % direction] = {"paths": paths, "fold": fold, "ld_const": ldc, "segments": [ns] + list(seg[:5 * max(ns, 0)])}
    return rec


def compute_all():
    from noise_flow_amd import _lib
    lib = _lib.load()
    keep = {k: os.environ.pop(k, None) for k in ENV_SWITCHES}
    out = {}
    try:
        for case in grid():
            env = case[-1]
            if env:
                name, value = env.split("=")
                os.environ[name] = value
            try:
                out[case_key(case)] = compute_case(lib, case)
            finally:
                if env:
                    del os.environ[name]
    finally:
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    return out


def test_every_layout_of_the_grid_is_bit_identical_to_the_recorded_builder():
    with open(GOLDEN) as f:
        golden = json.load(f)
    t0 = time.time()
    got = compute_all()
    print("fold-layout grid: %d cases in %.1f s" % (len(got), time.time() - t0))
    want = golden["cases"]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, "%d of %d cases differ from %s, first: %s\n got %r\nwant %r" % (
        len(bad), len(got), golden["recorded_from"], bad[0], got[bad[0]], want[bad[0]])
    # the grid reaches every family, every zero-padded width and every switch
    blocks = [0] * N_PATHS
    padded = set()
    for case in grid():
        for d in ("d0", "d1"):
            for path, v in enumerate(got[case_key(case)][d]["paths"]):
                if isinstance(v, str):
                    blocks[path] += 1
                    if path != 0 and case[3] in PADDED:
                        padded.add(case[3])
    assert min(blocks) >= 4, blocks
    assert padded == set(PADDED), sorted(set(PADDED) - padded)
    for name in ("NF_GEMM=a", "NF_GEMM16=a", "NF_H16=4x4"):   # a switch's cases must differ from the same cases without it
        hit = [c for c in grid() if c[-1] == name]
        assert hit and any(got[case_key(c)] != got[case_key(c[:-1] + ("",))] for c in hit), name
