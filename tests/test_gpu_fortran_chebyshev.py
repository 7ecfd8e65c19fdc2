"""The Chebyshev recurrence through the Fortran glue (gpu_chebyshev_moments_dev, gpu_chebyshev_apply_dev;
fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host (tests/fortran/chebyshev_check.f90, built by build_chebyshev_check() of
__graft_entry__.py) finds the ground state of the 2x2 plaquette's sector (2,2) on the device, makes v = c^+_{0,up} c_{1,up}|gs> and prints
12 moments of v with the probes (gs, v), the 23 self-moments, and for out = e^{-iHt} v its norm and its overlaps with the probes.  One
moments run and one apply run: they are the Python route's numbers to 1e-12 (the same library on the same vectors; values of order one), and
no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spin_pair_ref as S

pytestmark = pytest.mark.gpu


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_chebyshev_equals_the_python_route(built, tmp_path):
    import hxv
    from hxv import chebyshev as ch
    from oracle.oracle import OracleSector

    if not Path(built.FLANG).exists():
        pytest.skip("flang not available")
    exe = built.build_chebyshev_check()
    m, (N, _), _ = S.chi_fixture("plaquette")                    # Ns = 4, no bath; (2,2) has a non-degenerate ground state, Dim 36
    E = np.linalg.eigvalsh(OracleSector(m, N, N).dense())
    a, b = 0.5 * (E[-1] - E[0]) * 1.05, 0.5 * (E[-1] + E[0])
    coef = ch.propagator_coefficients(1.5, a, b)
    inp = tmp_path / "model.bin"
    with open(inp, "wb") as f:
        np.array([m.Nlat, m.Norb, m.Nspin, m.Nbath, N, N, int(m.hfmode)], dtype=np.int32).tofile(f)
        m.impHloc.ravel(order="F").tofile(f)
        m.Hbath.ravel(order="F").tofile(f)
        m.Vbath.ravel(order="F").tofile(f)
        np.concatenate([m.Uloc, [m.Ust, m.Jh, m.Jx, m.Jp, m.xmu]]).astype(np.float64).tofile(f)
        np.array([a, b], dtype=np.float64).tofile(f)
        np.array([len(coef)], dtype=np.int32).tofile(f)
        coef.astype(np.complex128).tofile(f)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = out.stdout

    sec = hxv.HxvSector.from_model(m, N, N)
    assert sec.Dim == 36
    e0, psi, _ = sec.lanczos_eigh(512, 1e-14, native=True)
    v, _, _ = sec.apply_one_body([(0, 0, 1, 1.0)], psi, subtract_mean=False)
    mom, smom = sec.chebyshev_moments(v, [psi, v], 12, a, b)
    res, n2 = sec.chebyshev_apply(v, coef, a, b)
    ov, _ = sec.chebyshev_moments(res, [psi, v], 1, a, b)
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert abs(_floats(txt, "E0")[0] - e0) <= 1e-12
    got_mom = (_floats(txt, "mom_re") + 1j * _floats(txt, "mom_im")).reshape((2, 12), order="F").T      # Fortran (probe, order) -> [order, probe]
    got_ov = _floats(txt, "ov")
    got_ov = got_ov[:2] + 1j * got_ov[2:]
    print(f"fortran - python: moments {np.abs(got_mom - mom).max():.3e} (max {np.abs(mom).max():.3e}), self-moments "
          f"{np.abs(_floats(txt, 'self') - smom).max():.3e}, norm2 {abs(_floats(txt, 'norm2')[0] - n2):.3e}, overlaps {np.abs(got_ov - ov[0]).max():.3e}")
    assert np.abs(mom).max() > 1e-2 and n2 > 1e-2
    assert np.abs(got_mom - mom).max() <= 1e-12 and np.abs(_floats(txt, "self") - smom).max() <= 1e-12
    assert abs(_floats(txt, "norm2")[0] - n2) <= 1e-12 and np.abs(got_ov - ov[0]).max() <= 1e-12
