"""The subset density matrix through the Fortran glue (gpu_reduced_dm_dev, fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host
(tests/fortran/reduced_dm_check.f90), compiled with build_fortran's compiler and link line, finds a ground state on the device, calls the
glue with a one-site mask and with the mask of the impurity bits {0,1} (the latter also accumulated in two halves in the Fermi-sign
convention) and prints trace, purity and matrix of each -- equal to the Python path on the same model and sector."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_reduced_dm_equals_the_python_path(built, tmp_path):
    import hxv
    from hxv import models

    ge = built
    if not Path(ge.FLANG).exists():
        pytest.skip("flang not available")
    lib = ge.build_engine()
    fdir = ge.PKG / "fortran"
    exe = tmp_path / "reduced_dm_check"
    subprocess.check_call([ge.FLANG, "-O2", "-J", str(tmp_path), "-o", str(exe), str(fdir / "ED_HAMILTONIAN_GPU_HxV.f90"),
                           str(ROOT / "tests" / "fortran" / "reduced_dm_check.f90"),
                           f"-L{lib.parent}", "-lhxv", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.15, hfmode=True)   # Ns = 6; sector (3,3) has a non-degenerate ground state
    nup, ndw = 3, 3
    inp = tmp_path / "model.bin"
    with open(inp, "wb") as f:
        np.array([m.Nlat, m.Norb, m.Nspin, m.Nbath, nup, ndw, int(m.hfmode)], dtype=np.int32).tofile(f)
        m.impHloc.ravel(order="F").tofile(f)
        m.Hbath.ravel(order="F").tofile(f)
        m.Vbath.ravel(order="F").tofile(f)
        np.concatenate([m.Uloc, [m.Ust, m.Jh, m.Jx, m.Jp, m.xmu]]).astype(np.float64).tofile(f)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = out.stdout

    sec = hxv.HxvSector.from_model(m, nup, ndw)
    ev, vecs, nc, _ = sec.eigh_lowest(1, tol=1e-14, native=True)
    psi = vecs[0].contiguous()
    site = np.zeros((m.Nlat, m.Norb), dtype=bool)
    site[0, :] = True
    want = {"site": sec.reduced_dm(psi, site), "pair": sec.reduced_dm(psi, (0, 1)), "fermi": sec.reduced_dm(psi, (0, 1), fermi_sign=True)}
    sec.close()
    assert abs(_floats(txt, "E0")[0] - ev[0]) < 1e-10
    assert np.abs(want["pair"] - np.diag(np.diag(want["pair"]))).max() > 1e-3          # off-diagonal weight is compared
    for tag, rho in want.items():
        assert abs(_floats(txt, tag + "_trace")[0] - np.trace(rho).real) < 1e-9 and abs(_floats(txt, tag + "_trace")[0] - 1.0) < 1e-9
        assert abs(_floats(txt, tag + "_purity")[0] - np.real(np.trace(rho @ rho))) < 1e-9
        assert np.abs(_floats(txt, tag + "_re") - rho.real.ravel(order="F")).max() < 1e-9
        assert np.abs(_floats(txt, tag + "_im") - rho.imag.ravel(order="F")).max() < 1e-9
