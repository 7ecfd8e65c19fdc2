"""The impurity observables through the Fortran glue (gpu_observables_dev / gpu_get_observables, fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small
flang host (tests/fortran/observables_check.f90), compiled with build_fortran's compiler and link line, finds a ground state on the device,
records it and derives dens, docc, Eknot -- equal to the Python path on the same model and sector."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_observables_equal_the_python_path(built, tmp_path):
    import hxv
    from hxv import models, observables

    ge = built
    if not Path(ge.FLANG).exists():
        pytest.skip("flang not available")
    lib = ge.build_engine()
    fdir = ge.PKG / "fortran"
    exe = tmp_path / "observables_check"
    subprocess.check_call([ge.FLANG, "-O2", "-J", str(tmp_path), "-o", str(exe), str(fdir / "ED_HAMILTONIAN_GPU_HxV.f90"),
                           str(ROOT / "tests" / "fortran" / "observables_check.f90"),
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
    rec = sec.observables_record(vecs[0].contiguous())
    sec.close()
    py = observables.derive(m, rec)
    assert abs(_floats(txt, "E0")[0] - ev[0]) < 1e-10
    assert np.abs(_floats(txt, "dens") - py["dens"].ravel(order="F")).max() < 1e-9
    assert np.abs(_floats(txt, "docc") - py["docc"].ravel(order="F")).max() < 1e-9
    assert abs(_floats(txt, "Eknot")[0] - py["Eknot"]) < 1e-9
    assert abs(_floats(txt, "Epot")[0] - py["Epot"]) < 1e-9
