"""Generate tests/golden/chamfer_sample_tri.npz from the reference's own `sample_single_tri`
(python/evaluate_chamfer_dtumvs.py:32-41).

    python tests/golden/make_chamfer_golden.py <path of the reference's python directory>

The reference module imports libraries that need not be installed where this runs (open3d, hydra, nnabla, omegaconf, tqdm,
sklearn) and its own `dataset` / `helper`; none of them is touched by `sample_single_tri`, so empty stand-ins are put into
`sys.modules` before the import.  The fixture holds recorded results only: for every (n1, n2) in {0, 1, 2, 3, 7, 16}^2 the
inputs (v1, v2, p0 drawn from a seeded generator) and the points the function returned, concatenated, with their counts.
(n1, n2) = (2, 2) has candidates whose k0 + k1 is exactly 1, (3, 3) candidates where it is 1 up to rounding."""
import importlib
import os
import sys
import types

import numpy as np

NS = (0, 1, 2, 3, 7, 16)
SEED = 20240229


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


def import_reference(ref_python):
    for name in ("open3d", "hydra", "nnabla", "omegaconf", "tqdm", "sklearn"):
        try:
            importlib.import_module(name)
        except ImportError:
            _stub(name)
    if not hasattr(sys.modules["nnabla"], "monitor"):
        sys.modules["nnabla"].monitor = _stub("nnabla.monitor", Monitor=object, MonitorSeries=object)
    if not hasattr(sys.modules["omegaconf"], "DictConfig"):
        sys.modules["omegaconf"].DictConfig = dict
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = object
    if not hasattr(sys.modules["sklearn"], "neighbors"):
        sys.modules["sklearn"].neighbors = _stub("sklearn.neighbors")
    _stub("dataset", IDRDataSource=object)
    _stub("helper", setup_system=lambda conf: None, watch_etime=lambda fn: fn)
    sys.path.insert(0, ref_python)
    return importlib.import_module("evaluate_chamfer_dtumvs")


def main():
    ref = import_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    n, v1, v2, p0, counts, points = [], [], [], [], [], []
    for n1 in NS:
        for n2 in NS:
            a, b, c = rng.standard_normal((3, 3)) * np.array([[1.0], [0.7], [3.0]])
            q = ref.sample_single_tri((np.float64(n1), np.float64(n2), a[None, :], b[None, :], c))
            n.append((n1, n2)); v1.append(a); v2.append(b); p0.append(c)
            counts.append(q.shape[0]); points.append(q.reshape(-1, 3))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chamfer_sample_tri.npz")
    np.savez_compressed(out, n=np.asarray(n, dtype=np.int64), v1=np.asarray(v1), v2=np.asarray(v2), p0=np.asarray(p0),
                        counts=np.asarray(counts, dtype=np.int64), points=np.concatenate(points, axis=0))
    print(out, sum(counts), "points")


if __name__ == "__main__":
    main()
