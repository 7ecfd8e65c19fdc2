"""One-body operators through the Fortran glue (gpu_apply_one_body_dev, gpu_sp_lanc_tridiag_probes_dev, gpu_gf_from_probes;
fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host (tests/fortran/one_body_check.f90, built by build_one_body_check() of
__graft_entry__.py) finds the ground state of the 2x2 plaquette's sector (2,2) on the device and prints the means and fluctuation norms of
the bond and current operators of orbitals (0,1), the mean of a single hop, and chi(i nu_n) for n = 0, 1, 5 at beta = 50; they are the
Python route's to 1e-12, and no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import one_body_ref as R
import spin_pair_ref as S

pytestmark = pytest.mark.gpu


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_one_body_chi_equals_the_python_route(built, tmp_path):
    import hxv
    from hxv import observables

    if not Path(built.FLANG).exists():
        pytest.skip("flang not available")
    exe = built.build_one_body_check()
    m, (N, _), _ = S.chi_fixture("plaquette")                    # Ns = 4, no bath; (2,2) has a non-degenerate ground state, Dim 36
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

    sec = hxv.HxvSector.from_model(m, N, N)
    assert sec.Dim == 36
    e0, psi, _ = sec.lanczos_eigh(512, 1e-14, native=True)
    nu = 2.0 * np.pi * np.array([0, 1, 5]) / 50.0
    ops = [R.bond(0, 1), R.current(0, 1)]
    chi, info = observables.one_body_susceptibility(sec, psi, e0, ops, 1j * nu, nlanc=36)
    _, hop_mean, hop_n2 = sec.apply_one_body([(0, 0, 1, 1.0)], psi, subtract_mean=False)
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert abs(_floats(txt, "E0")[0] - e0) <= 1e-12
    got = (_floats(txt, "chi_re") + 1j * _floats(txt, "chi_im")).reshape((3, 2, 2), order="F")
    mean, n2, hop = _floats(txt, "mean_re") + 1j * _floats(txt, "mean_im"), _floats(txt, "norm2"), _floats(txt, "hop")
    print(f"fortran - python: mean {np.abs(mean - info['mean'][0]).max():.3e}, norm2 {np.abs(n2 - info['norm2'][0]).max():.3e}, "
          f"chi {np.abs(got - chi).max():.3e} (max |chi| {np.abs(chi).max():.3e})")
    assert np.abs(chi).max() > 1e-2 and abs(hop_mean) > 1e-2
    assert np.abs(mean - info["mean"][0]).max() <= 1e-12 and np.abs(n2 - info["norm2"][0]).max() <= 1e-12
    assert abs(complex(hop[0], hop[1]) - hop_mean) <= 1e-12 and abs(hop[2] - hop_n2) <= 1e-12
    assert np.abs(got - chi).max() <= 1e-12
