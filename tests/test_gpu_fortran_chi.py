"""The susceptibility stage through the Fortran glue (gpu_apply_density_ops_dev, gpu_sp_lanc_tridiag_probes_dev, gpu_gf_from_probes;
fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host (tests/fortran/chi_check.f90), compiled with build_fortran's compiler and link line,
finds the ground state of the Ns = 6 chain's sector (3,3) on the device and prints the means and norms of dS^z_a|gs> and chi_spin(i nu_n) for
n = 0, 1, 5 at beta = 50; they are the Python route's to 1e-12, and no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_chi_equals_the_python_route(built, tmp_path):
    import hxv
    from hxv import models, observables

    ge = built
    if not Path(ge.FLANG).exists():
        pytest.skip("flang not available")
    lib = ge.build_engine()
    fdir = ge.PKG / "fortran"
    exe = tmp_path / "chi_check"
    subprocess.check_call([ge.FLANG, "-O2", "-J", str(tmp_path), "-o", str(exe), str(fdir / "ED_HAMILTONIAN_GPU_HxV.f90"),
                           str(ROOT / "tests" / "fortran" / "chi_check.f90"),
                           f"-L{lib.parent}", "-lhxv", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0)     # Ns = 6; (3,3) has a non-degenerate ground state
    N = 3
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
    e0, psi, _ = sec.lanczos_eigh(512, 1e-14, native=True)
    nu = 2.0 * np.pi * np.array([0, 1, 5]) / 50.0
    chi, info = observables.susceptibility(sec, psi, e0, "spin", 1j * nu)
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert abs(_floats(txt, "E0")[0] - e0) <= 1e-12
    # (the ground state comes back with the same global sign from the same deterministic start vector; chi is bilinear in it anyway)
    got = (_floats(txt, "chi_re") + 1j * _floats(txt, "chi_im")).reshape((3, 2, 2), order="F")
    print(f"fortran - python: mean {np.abs(_floats(txt, 'mean') - info['mean']).max():.3e}, norm2 {np.abs(_floats(txt, 'norm2') - info['norm2']).max():.3e}, "
          f"chi {np.abs(got - chi).max():.3e} (max |chi| {np.abs(chi).max():.3e})")
    assert np.abs(chi).max() > 0.1
    assert np.abs(_floats(txt, "mean") - info["mean"]).max() <= 1e-12 and np.abs(_floats(txt, "norm2") - info["norm2"]).max() <= 1e-12
    assert np.abs(got - chi).max() <= 1e-12
