"""Make tests/golden/g19_verify.npz: what the REFERENCE's utils.metrics.Metrics makes of the forecast-verification
cases of tests/_verify_ref.py (CASES). CPU only; needs the reference tree that oracle.ref_harness imports (it is not
part of this repository).

    python tools/make_verify_fixture.py

Per case every Metrics method vv_verify mirrors is run on the fp32-normalised fields with data_std = scale, once in
fp32 (stored as <case>_<name>, a (C,) float64 array; MSE and MAE, Python floats in the reference, repeated C times)
and once on the same fields cast to float64; <case>_spread_<name> = max |fp32 - fp64| / max |fp64| is the
reference's own rounding spread, asserted below 3e-7 (a case that exceeds it gets another seed, not a wider bound).
The small cases also store their inputs; the workload case's are regenerated from its seed by make_case. Only data is
written."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-var_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SPREAD_BOUND = 3e-7


def main():
    import torch

    from oracle import ref_harness

    ref_harness.import_reference()
    M = importlib.import_module("utils.metrics").Metrics()
    from _verify_ref import CASES, NAMES, STORED_INPUTS, make_case, normalise

    out = {}
    for case in CASES:
        d = make_case(case)
        pn, tn, cn = (normalise(d[k], d["mean"], d["std"]) for k in ("pred", "gt", "clim"))
        scale = torch.from_numpy(d["scale"])
        C = pn.shape[1]
        worst = 0.0
        for name in NAMES:
            r = {}
            for dt in (torch.float32, torch.float64):
                v = getattr(M, name)(pn.to(dt), tn.to(dt), None, cn.to(dt), scale)
                v = v.detach().double().numpy() if isinstance(v, torch.Tensor) else np.full(C, v, np.float64)
                assert v.shape == (C,), (name, v.shape)
                r[dt] = v
            spread = float(np.max(np.abs(r[torch.float32] - r[torch.float64])) / np.max(np.abs(r[torch.float64])))
            assert spread < SPREAD_BOUND, (case, name, spread)
            worst = max(worst, spread)
            out[f"{case}_{name}"] = r[torch.float32]
            out[f"{case}_spread_{name}"] = np.float64(spread)
        if case in STORED_INPUTS:
            for k, v in d.items():
                out[f"{case}_{k}"] = v
        print(case, CASES[case], "largest fp32-vs-fp64 spread %.2e" % worst)
    path = os.path.join(ROOT, "tests", "golden", "g19_verify.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
