"""The twin-sector map through the Fortran glue (gpu_twin_vector, fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host
(tests/fortran/twin_check.f90), compiled with build_fortran's compiler and link line, finds the ground state of (2,4) on the device, keeps the
sector, opens (4,2), maps the state into it and tridiagonalises from there -- alanc(1) is the ground-state energy again, the amplitudes are the
Python path's, and no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_twin_vector_equals_the_python_path(built, tmp_path):
    import hxv
    from hxv import models

    ge = built
    if not Path(ge.FLANG).exists():
        pytest.skip("flang not available")
    lib = ge.build_engine()
    fdir = ge.PKG / "fortran"
    exe = tmp_path / "twin_check"
    subprocess.check_call([ge.FLANG, "-O2", "-J", str(tmp_path), "-o", str(exe), str(fdir / "ED_HAMILTONIAN_GPU_HxV.f90"),
                           str(ROOT / "tests" / "fortran" / "twin_check.f90"),
                           f"-L{lib.parent}", "-lhxv", f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    m = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2], xmu=0.15)   # Ns = 6; (2,4) has a non-degenerate ground state
    nup, ndw = 2, 4
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

    a, b = hxv.HxvSector.from_model(m, nup, ndw), hxv.HxvSector.from_model(m, ndw, nup)
    ev, vecs, nc, _ = a.eigh_lowest(1, 20, tol=1e-14, native=True)
    amp = b.vector_to_host(a.twin_vector(b, vecs[0].contiguous()))[:16]
    a.close()
    b.close()
    e0, a1 = _floats(txt, "E0")[0], _floats(txt, "alanc1")[0]
    got = _floats(txt, "amp_re") + 1j * _floats(txt, "amp_im")
    print("E0", e0, "alanc(1) - E0", a1 - e0, "E0 - python", e0 - ev[0])
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert abs(e0 - ev[0]) < 1e-10
    assert abs(a1 - e0) < 1e-10
    assert np.abs(amp).max() > 0.1                                       # the printed amplitudes carry weight
    k = int(np.argmax(np.abs(amp)))
    sign = np.sign((got[k] * np.conj(amp[k])).real)                      # the one global sign of the eigenvector
    assert sign != 0 and np.abs(got - sign * amp).max() < 1e-9
