"""The real-vector Chebyshev recurrence and the seeded random device state through the Fortran glue (gpu_vector_random_dev,
gpu_chebyshev_moments_real_dev, gpu_chebyshev_apply_real_dev; fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host
(tests/fortran/chebyshev_real_check.f90, built by build_chebyshev_real_check() of __graft_entry__.py) makes two random vectors v, p on the
device in a real-H sector where real vectors are available -- the 2x2 plaquette's (2,2) when they are there, otherwise the Ns = 6 chain's
(3,3) -- and prints 12 real moments of v with the probes (p, v), the 23 self-moments, and for out = e^{-tau H} v its norm and its overlaps
with the probes.  They are the Python route's numbers to 1e-12 (the same library on the same vectors; the bound of
tests/test_gpu_fortran_chebyshev.py), and no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spin_pair_ref as S

pytestmark = pytest.mark.gpu

SEED = 2024


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_chebyshev_real_equals_the_python_route(built, tmp_path):
    import hxv
    from hxv import chebyshev as ch, models
    from oracle.oracle import OracleSector

    if not Path(built.FLANG).exists():
        pytest.skip("flang not available")
    exe = built.build_chebyshev_real_check()
    m, (N, _), _ = S.chi_fixture("plaquette")
    sec = hxv.HxvSector.from_model(m, N, N)
    if not sec.real_vectors_available:
        sec.close()
        m, N = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), 3
        sec = hxv.HxvSector.from_model(m, N, N)
    assert sec.real_vectors_available
    E = np.linalg.eigvalsh(OracleSector(m, N, N).dense())
    a, b = 0.5 * (E[-1] - E[0]) * 1.05, 0.5 * (E[-1] + E[0])
    coef = ch.exp_coefficients(0.7, a, b).real.copy()
    inp = tmp_path / "model.bin"
    with open(inp, "wb") as f:
        np.array([m.Nlat, m.Norb, m.Nspin, m.Nbath, N, N, int(m.hfmode)], dtype=np.int32).tofile(f)
        m.impHloc.ravel(order="F").tofile(f)
        m.Hbath.ravel(order="F").tofile(f)
        m.Vbath.ravel(order="F").tofile(f)
        np.concatenate([m.Uloc, [m.Ust, m.Jh, m.Jx, m.Jp, m.xmu]]).astype(np.float64).tofile(f)
        np.array([a, b], dtype=np.float64).tofile(f)
        np.array([len(coef)], dtype=np.int32).tofile(f)
        coef.astype(np.float64).tofile(f)
        np.array([SEED], dtype=np.int64).tofile(f)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = out.stdout

    v, p = sec.random_vector(SEED), sec.random_vector(SEED + 1)
    mom, smom = sec.chebyshev_moments_real(v, [p, v], 12, a, b)
    res, n2 = sec.chebyshev_apply_real(v, coef, a, b)
    ov, _ = sec.chebyshev_moments_real(res, [p, v], 1, a, b)
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    got_mom = _floats(txt, "mom").reshape((2, 12), order="F").T      # Fortran (probe, order) -> [order, probe]
    got_ov = _floats(txt, "ov")
    print(f"fortran - python: moments {np.abs(got_mom - mom).max():.3e} (max {np.abs(mom).max():.3e}), self-moments "
          f"{np.abs(_floats(txt, 'self') - smom).max():.3e}, norm2 {abs(_floats(txt, 'norm2')[0] - n2):.3e}, overlaps {np.abs(got_ov - ov[0]).max():.3e}")
    assert np.abs(mom).max() > 1e-2 and n2 > 1e-2
    assert np.abs(got_mom - mom).max() <= 1e-12 and np.abs(_floats(txt, "self") - smom).max() <= 1e-12
    assert abs(_floats(txt, "norm2")[0] - n2) <= 1e-12 and np.abs(got_ov - ov[0]).max() <= 1e-12
