"""What the host side of the library makes of every layer kind, one line per case, for a before / after comparison of a change
that should move code only (CPU only: nf_layer_param_count, nf_fold_params and nf_cond_rows need no device).

    NF_TOOL_LIB=build/variants/lib_<parent>.so python tools/layer_vocab_dump.py > parent.txt
    python tools/layer_vocab_dump.py --against parent.txt > profiles/<name>.txt

Cases: nf_layer_param_count of every kind (and two numbers that are none) at widths 1, 4, 5, 32 and 512; one model `<kind>|unc`
per sdn / gain kind and 1x1 setting (PLU, LU2, NONE, permutation), width 4 on 8x8 patches: nf_fold_params in both directions (ops,
folded block, constant log-det) and nf_cond_rows in both directions at the five table ISOs and ISO 250, cameras 0 .. 4.  A line
holds the SHA-256 of the bytes the call wrote; --against marks every line `same` or `DIFFERS` and exits 1 on a difference."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from noise_flow_amd import _lib, params  # noqa: E402

if os.environ.get("NF_TOOL_LIB"):   # A/B a differently-built library (this tool only)
    _lib.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])

KINDS = ["sdn5", "sdn4", "gain4", "sdn", "gain", "sdn1", "sdn2", "sdn3", "sdn6", "gain1", "gain2", "gain3"]
SETTINGS = [(1, "LU"), (1, "LU2"), (1, "NONE"), (0, "LU")]
ISOS = [100, 400, 800, 1600, 3200, 250]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def lines():
    from conftest import trained_like_variables
    from test_gpu_random_sweep import _condition
    lib = _lib.load()
    for w in (1, 4, 5, 32, 512):
        yield "param_count width %d: %s" % (w, " ".join(str(lib.nf_layer_param_count(t, w)) for t in range(0, 19)))
    for kind in KINDS:
        for fp, decomp in SETTINGS:
            arch, seed = kind + "|unc", 11 + KINDS.index(kind)
            v = params.init_variables(arch, 4, 4, seed, fp, decomp)
            v.update({k: a for k, a in trained_like_variables(arch, 4, seed=seed).items() if k in v})
            v = _condition(v, arch, 4, 800, np.random.RandomState(seed))
            layers, descs, flat = params.pack(arch, v, 4, "loss_first", fp, decomp)
            cfg = _lib.nf_config(8, 8, 4, len(layers), -1, 0)
            fptr = flat.ctypes.data_as(C.POINTER(C.c_float))
            name = "%s fp=%d %s" % (arch, fp, decomp)
            for direction in (0, 1):
                n_ops, n_folded, ld = C.c_int32(0), C.c_size_t(0), C.c_double(0.0)
                rc = lib.nf_fold_params(C.byref(cfg), descs, fptr, flat.size, direction, None, 0, C.byref(n_ops), None, 0, C.byref(n_folded), C.byref(ld))
                assert rc == 0, (name, lib.nf_last_error())
                ops, blk = np.zeros(2 * n_ops.value, np.int32), np.zeros(n_folded.value, np.float32)
                rc = lib.nf_fold_params(C.byref(cfg), descs, fptr, flat.size, direction, ops.ctypes.data_as(C.POINTER(C.c_int32)), n_ops.value,
                                        C.byref(n_ops), blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(n_folded), C.byref(ld))
                assert rc == 0, (name, lib.nf_last_error())
                yield "%s fold dir %d: %d ops, %d floats, %s" % (name, direction, n_ops.value, blk.size, sha(ops, blk, np.float64(ld.value)))
                conds = (_lib.nf_cond * (len(ISOS) * 5))(*[_lib.nf_cond(float(iso), float(cam), 0.0, 0.0) for iso in ISOS for cam in range(5)])
                rows = (_lib.nf_cond_row * len(conds))()
                rc = lib.nf_cond_rows(C.byref(cfg), descs, fptr, flat.size, direction, conds, len(conds), rows)
                assert rc == 0, (name, lib.nf_last_error())
                yield "%s cond_rows dir %d: %d rows, %s" % (name, direction, len(conds), sha(np.frombuffer(rows, np.uint8)))


def main():
    got = list(lines())
    if "--against" not in sys.argv:
        print("\n".join(got))
        return 0
    want = open(sys.argv[sys.argv.index("--against") + 1]).read().splitlines()
    bad = 0
    for i, g in enumerate(got):
        same = i < len(want) and want[i] == g
        bad += not same
        print("%s  %s" % (g, "same" if same else "DIFFERS"))
    bad += len(want) != len(got)
    print("%d cases, %d differ from %s" % (len(got), bad, "the other build"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
