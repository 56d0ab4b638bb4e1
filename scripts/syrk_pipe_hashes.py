"""sha256 of every output table of the SYRK-pipelining cases, with the library
in the tree.

The split-bf16 SYRK's operand reads were moved relative to its MFMAs without
touching the arithmetic, so the outputs must be the same bits as the parent
commit's.  This script runs the cases and prints their hashes as JSON;
`--write [PATH] --commit HASH` stores them (tests/golden/
syrk_pipe_parent_sha256.json is such a run of the parent's library), and
tests/test_syrk_pipe_gpu.py compares the tree's library against that file.

Cases: one half-step on tests/seam_data.py for keys x dims x modes (the
modes are test_seam_gpu's environments; hspace_max does not exist at Dp = 32,
as there), and the two-epoch iALS trajectory of scripts/bitwise_epochs.py at
d = 256 under the default dispatch.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "safer2-recommender_amd"),
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "syrk_pipe_parent_sha256.json")

KEYS = ["ials_user", "ials_item", "weighted_u", "weighted_v_quirk"]
PADDED = {20: 32, 64: 64, 100: 128, 200: 224, 256: 256}  # dim: Dp, T = 1, 2, 4, 7, 8
DIMS = list(PADDED)
MODES = ["dspace", "dspace_split", "hspace_max"]
EPOCH_DIM = 256


def mode_env(mode, Dp):
    """test_seam_gpu._mode_env for the three modes used here."""
    if mode == "dspace":
        return {"FRECSYS_DUAL": "0"}
    if mode == "dspace_split":
        return {"FRECSYS_DUAL": "0", "FRECSYS_SPLIT_ROWS": "64"}
    if mode == "hspace_max":
        return {"FRECSYS_DUAL_MAX_H": "256"} if 64 <= Dp <= 256 else None
    raise ValueError(mode)


def seam_cases():
    return [(k, d, m) for m in MODES for d in DIMS for k in KEYS
            if mode_env(m, PADDED[d]) is not None]


def case_id(key, dim, mode):
    return f"seam/{key}/d{dim}/{mode}"


def case_ids():
    return [case_id(*c) for c in seam_cases()] + [f"epochs/ials_d{EPOCH_DIM}/{t}" for t in "UV"]


class _Env:
    """The process environment with every FRECSYS_* dropped and `env` set."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: v for k, v in os.environ.items() if k.startswith("FRECSYS_")}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)
        os.environ.update(self.saved)


def run_seam(key, dim, mode):
    """The half-step of test_seam_gpu._gpu_run; returns the solved table."""
    import frecsys_hip as fh
    import seam_data as S
    c = S.seam_case(key, dim)
    assert fh.padded_dim(dim) == PADDED[dim]
    with _Env(mode_env(mode, PADDED[dim])):
        ctx = fh.Context(dim, c.nu, c.ni, parity_quirks=c.quirk)
        ctx.load_csr(fh.SIDE_USER, c.up, c.uc)
        ctx.load_csr(fh.SIDE_ITEM, c.ip, c.ic)
        ctx.set_embeddings(fh.SIDE_USER, c.U)
        ctx.set_embeddings(fh.SIDE_ITEM, c.V)
        side, other = ((fh.SIDE_USER, fh.SIDE_ITEM) if c.seam == "user"
                       else (fh.SIDE_ITEM, fh.SIDE_USER))
        ctx.gramian(other, weights=c.gram_weights, fetch=False)
        if c.kind == fh.KIND_IALS:
            kw = dict(reg_exp=c.reg_exp)
        elif c.kind == fh.KIND_WEIGHTED_U:
            kw = dict(entity_weight=c.entity_weight)
        else:
            kw = dict(alpha=c.alpha, entity_reg=c.entity_reg, other_weight=c.other_weight)
        ctx.solve_side(side, c.kind, c.reg, c.w, **kw)
        out = ctx.get_embeddings(side)
        ctx.close()
    return out


def run_epochs(dim=EPOCH_DIM):
    """scripts/bitwise_epochs.py at one dim: two iALS epochs on quirk_data."""
    import frecsys_hip as fh
    import oracle as O
    from conftest import make_quirk_data
    nu, ni, up, uc, ip, ic = make_quirk_data()
    with _Env({}):
        ctx = fh.Context(dim, nu, ni, parity_quirks=True)
        ctx.load_csr(fh.SIDE_USER, up, uc)
        ctx.load_csr(fh.SIDE_ITEM, ip, ic)
        U, V = O.init_embeddings(1, 0.1, dim, nu, ni)
        ctx.set_embeddings(fh.SIDE_USER, U)
        ctx.set_embeddings(fh.SIDE_ITEM, V)
        for _ in range(2):
            ctx.gramian(fh.SIDE_ITEM)
            ctx.solve_side(fh.SIDE_USER, fh.KIND_IALS, 0.003, 0.1)
            ctx.gramian(fh.SIDE_USER)
            ctx.solve_side(fh.SIDE_ITEM, fh.KIND_IALS, 0.003, 0.1)
        U, V = ctx.get_embeddings(fh.SIDE_USER), ctx.get_embeddings(fh.SIDE_ITEM)
        ctx.close()
    return U, V


def digest(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def all_hashes():
    h = {}
    for key, dim, mode in seam_cases():
        h[case_id(key, dim, mode)] = digest(run_seam(key, dim, mode))
    U, V = run_epochs()
    h[f"epochs/ials_d{EPOCH_DIM}/U"] = digest(U)
    h[f"epochs/ials_d{EPOCH_DIM}/V"] = digest(V)
    return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", nargs="?", const=GOLDEN, default=None, metavar="PATH",
                    help="store the hashes (default: the golden file of the test)")
    ap.add_argument("--commit", default=None, help="commit hash of the library that ran (recorded)")
    ap.add_argument("--check", default=None, metavar="PATH",
                    help="compare with a stored file; exit 1 on any difference")
    a = ap.parse_args()
    doc = {"commit": a.commit, "hashes": all_hashes()}
    print(json.dumps(doc, indent=1))
    if a.write:
        with open(a.write, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if a.check:
        with open(a.check) as f:
            want = json.load(f)["hashes"]
        diff = sorted(k for k in set(want) | set(doc["hashes"]) if want.get(k) != doc["hashes"].get(k))
        print(f"{len(diff)} of {len(want)} differ from {a.check}: {diff}")
        sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
