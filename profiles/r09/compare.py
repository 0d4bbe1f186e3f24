"""compare.py A.npz B.npz [TOL]: every array of A against B.  Without TOL np.array_equal is required; with TOL an array that
differs passes when max |a - b| <= TOL max |b| and is named.  Exit status 1 when an array fails or the two files hold different
arrays."""
import sys

import numpy as np

a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
tol = float(sys.argv[3]) if len(sys.argv) > 3 else None
bad = sorted(set(a.files) ^ set(b.files))
differ = []
for k in sorted(set(a.files) & set(b.files)):
    if a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True):
        continue
    err = np.abs(a[k] - b[k]).max() / max(np.abs(b[k]).max(), 1e-300) if a[k].shape == b[k].shape else np.inf
    differ.append((k, err))
    if tol is None or not err <= tol:
        bad.append(k)
for k, err in differ:
    print(f"  differs: {k} {err:.3e}")
print(f"{sys.argv[1]} vs {sys.argv[2]}: {len(a.files)} arrays, {len(differ)} differ, {len(bad)} fail")
sys.exit(1 if bad else 0)
