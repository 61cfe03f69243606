"""Copies the reference's B-matrix statistics (dataset/bq_info_lr/*.npy: data, not code) into the committed fixture
tests/golden/bq_info_lr.npz, so the sc4dvar parity tests run where /root/reference is absent (the GPU box).
Loaded with allow_pickle=False. Usage: python -B oracle/make_bq_fixture.py"""
import hashlib
import json
import os
import sys

import numpy as np

SRC = "/root/reference/dataset/bq_info_lr"
DST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "bq_info_lr.npz")
KEYS = ("len_scale", "reg_coeff", "std_sur", "vert_eig_value", "vert_eig_vec")

if __name__ == "__main__":
    if not os.path.isdir(SRC):
        sys.exit(f"{SRC} not found")
    src = {k: np.load(os.path.join(SRC, k + ".npy"), allow_pickle=False) for k in KEYS}
    np.savez(DST, **src)
    print("wrote", DST)
    # the digests of the source files' arrays, which tests/test_sc4dvar_oracle.py holds the fixture against
    digests = {k: {"sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), "shape": list(a.shape),
                   "dtype": str(a.dtype)} for k, a in src.items()}
    with open(DST[:-len(".npz")] + ".sha256.json", "w") as f:
        json.dump(digests, f, indent=1)
        f.write("\n")
    print("wrote", f.name)
