"""Writes tests/golden/match_parent.npz: what egonn_match_mutual gave on an MI355X AT COMMIT a2c5576, the parent of the
refactor that put one tile / merge kernel pair behind both matching entry points.  Until then egonn_match_mutual ran
reg_match_kernel (one workgroup per pair, the distance table computed once per direction), so the recorded results are an
implementation independent of the kernels the tests run today.  Runs on a checkout of that commit with this script and
tests/match_data.py copied onto it (it calls egonn_amd.match_mutual, whose Python signature did not change), on the device:

    python tests/golden/make_golden_match.py --commit $(git rev-parse HEAD)

Per set of tests/match_data.py (every indexed set in its gathered form, every dense set as it is): `<name>.corr` (P, n_max, 2)
int32, `<name>.n_corr` (P,) int32 and `<name>.sha256`, the hash of the input arrays; `commit`.  Only indices and hashes are
stored."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import match_data as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the checkout this runs on (the parent of the refactor)")
    ap.add_argument("--out", default=D.GOLDEN)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the recorded results come from the device"
    import __graft_entry__ as g
    g.build()
    import egonn_amd
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    out = {"commit": np.array(args.commit)}
    sets = [(name, D.dense_of(*s), s) for name, s in D.index_sets().items()]
    sets += [(name, s, s) for name, s in D.dense_sets().items()]
    for name, (F1, F2, n1, n2), hashed in sets:
        corr, n_corr = egonn_amd.match_mutual(cu(F1), cu(F2), cu(n1), cu(n2))
        torch.cuda.synchronize()
        out[name + ".corr"], out[name + ".n_corr"] = corr.cpu().numpy(), n_corr.cpu().numpy()
        out[name + ".sha256"] = np.array(D.input_sha256(hashed))
        print(f"{name}: {len(F1)} pairs, n_corr {out[name + '.n_corr'].tolist()}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
