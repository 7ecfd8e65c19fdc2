"""The pair susceptibility through the Fortran glue (gpu_apply_spin_pair_dev, gpu_sp_lanc_tridiag_probes_dev, gpu_gf_from_probes;
fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host (tests/fortran/spin_pair_check.f90, built by build_spin_pair_check() of
__graft_entry__.py) finds the ground state of the Ns = 6 chain's sector (3,3) on the device, keeps it, and prints the norms of O_a|gs>,
O_a^+|gs> and the local pair susceptibility chi(i nu_n) for n = 0, 1, 5 at beta = 50; they are the Python route's to 1e-12, and no sector
is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spin_pair_ref as R

pytestmark = pytest.mark.gpu


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_pair_chi_equals_the_python_route(built, tmp_path):
    import hxv
    from hxv import observables

    if not Path(built.FLANG).exists():
        pytest.skip("flang not available")
    exe = built.build_spin_pair_check()
    m, (N, _), _ = R.chi_fixture("chain")                         # Ns = 6; (3,3) has a non-degenerate ground state
    inp = tmp_path / "model.bin"
    with open(inp, "wb") as f:
        np.array([m.Nlat, m.Norb, m.Nspin, m.Nbath, N, N, int(m.hfmode)], dtype=np.int32).tofile(f)
        m.impHloc.ravel(order="F").tofile(f)
        m.Hbath.ravel(order="F").tofile(f)
        m.Vbath.ravel(order="F").tofile(f)
        np.concatenate([m.Uloc, [m.Ust, m.Jh, m.Jx, m.Jp, m.xmu]]).astype(np.float64).tofile(f)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = out.stdout

    sec, lo, up = (hxv.HxvSector.from_model(m, N + d, N + d) for d in (0, -1, 1))
    e0, psi, _ = sec.lanczos_eigh(512, 1e-14, native=True)
    nu = 2.0 * np.pi * np.array([0, 1, 5]) / 50.0
    chi, info = observables.spin_pair_susceptibility(sec, lo, up, psi, e0, observables.spin_pair_terms("local_pair", 2), False, False, 1j * nu, nlanc=400)
    for s in (sec, lo, up):
        s.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert abs(_floats(txt, "E0")[0] - e0) <= 1e-12
    got = (_floats(txt, "chi_re") + 1j * _floats(txt, "chi_im")).reshape((3, 2, 2), order="F")
    n2 = _floats(txt, "norm2").reshape((2, 2), order="F")        # (operator, side): side 1 = O^+, 2 = O
    print(f"fortran - python: norm2 {max(np.abs(n2[:, 0] - info['norm2_raise']).max(), np.abs(n2[:, 1] - info['norm2_lower']).max()):.3e}, "
          f"chi {np.abs(got - chi).max():.3e} (max |chi| {np.abs(chi).max():.3e})")
    assert np.abs(chi).max() > 1e-2
    assert np.abs(n2[:, 0] - info["norm2_raise"]).max() <= 1e-12 and np.abs(n2[:, 1] - info["norm2_lower"]).max() <= 1e-12
    assert np.abs(got - chi).max() <= 1e-12
