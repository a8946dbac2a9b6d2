"""Worker of tests/test_gpu_blockeval.py::test_user_kind_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_eval_blocks for a residual kind
that exists only as a device template of a USER header (tests/user_kinds/radial_ba.hpp, NLLS_RES_USER0: an affine camera with one radial distortion coefficient) -- no
oracle has the kind, so the reference is a numpy restatement of that one header, and the kernel values come from the closed forms of src/robust.jl:47-55.
Tolerances as in tests/test_gpu_blockeval.py."""
import math
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_gpu_blockeval.py"
USER0 = 100
K.register_user_kind(USER0, 2, 2, 2, ((K.VAR_EUCLIDEAN, 7), (K.VAR_EUCLIDEAN, 3)))


def main():
    rng = np.random.default_rng(21); ncam, npts, percam = 12, 300, 4
    p = N.NLLSProblem()
    cams = [p.addvariable(np.concatenate([rng.standard_normal(6) * 0.3 + np.array([1, 0, 0, 0, 1, 0.0]), [0.02 * rng.standard_normal()]])) for _ in range(ncam)]
    pts = [p.addvariable(rng.uniform(-0.5, 0.5, 3) + np.array([0, 0, 2.0])) for _ in range(npts)]
    vi = np.array([[cams[(j + k) % ncam], pts[j]] for j in range(npts) for k in range(percam)], np.int64)
    off = p.var_offsets; v = p.variables
    c = v[off[vi[:, 0] - 1][:, None] + np.arange(7)]; X = v[off[vi[:, 1] - 1][:, None] + np.arange(3)]
    def model(c, X):
        u = c[:, 0] * X[:, 0] + c[:, 1] * X[:, 1] + c[:, 2] * X[:, 2]; w = c[:, 3] * X[:, 0] + c[:, 4] * X[:, 1] + c[:, 5] * X[:, 2]
        s = c[:, 6] * (u * u + w * w) + 1.0
        return np.stack([s * u, s * w], 1)
    meas = model(c, X) + 1e-3 * rng.standard_normal((vi.shape[0], 2))
    meas[rng.random(vi.shape[0]) < 0.1] += 0.1
    width = 0.004
    p.addcosts(USER0, vi, meas, N.HuberKernel(width))
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups()); ctx.set_variables(p.variables)
    dev = ctx.eval_blocks(0)
    r = model(c, X) - meas; sq = (r * r).sum(1)
    inl = sq < width * width
    rho = np.where(inl, sq, 2 * width * np.sqrt(sq) - width * width); w = np.where(inl, 1.0, width / np.sqrt(np.maximum(sq, 1e-300)))
    scale = np.maximum(1.0, np.abs(meas).max(1))
    er = np.max(np.abs(dev["r"] - r) / scale[:, None])
    esq = np.max((np.abs(dev["sqerr"] - sq) - 1e-13 * scale ** 2) / sq)
    erho = np.max(np.abs(dev["rho"] - rho) / rho); ew = np.max(np.abs(dev["weight"] - w) / w)
    print(f"BLOCKEVAL user0: n={sq.size} outliers {int((~inl).sum())} r {er:.3e} sqerr {esq:.3e} rho {erho:.3e} weight {ew:.3e}")
    assert er <= 1e-13 and esq <= 1e-11 and erho <= 1e-11 and ew <= 1e-11
    assert 0 < (~inl).sum() < sq.size
    total = 0.5 * math.fsum(dev["rho"].tolist())
    assert np.isclose(total, ctx.sweep_cost(), rtol=1e-11)
    ctx.close()
    print("user kind block values ok")


if __name__ == "__main__":
    main()
