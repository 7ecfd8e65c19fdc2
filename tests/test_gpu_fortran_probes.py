"""Probe overlaps through the Fortran glue (gpu_sp_lanc_tridiag_probes_dev, gpu_gf_from_probes; fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small
flang host (tests/fortran/probes_check.f90), compiled with build_fortran's compiler and link line, computes the particle part of G_01 of the
Ns = 6 chain from ONE run -- ground state of (3,3) on the device, c^dagger_0|gs> as start vector, c^dagger_1|gs> as probe -- and prints poles and
weights; they are the Python path's, and no sector is left open."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_probes_equal_the_python_path(built, tmp_path):
    import hxv
    from hxv import greens, models

    ge = built
    if not Path(ge.FLANG).exists():
        pytest.skip("flang not available")
    lib = ge.build_engine()
    fdir = ge.PKG / "fortran"
    exe = tmp_path / "probes_check"
    subprocess.check_call([ge.FLANG, "-O2", "-J", str(tmp_path), "-o", str(exe), str(fdir / "ED_HAMILTONIAN_GPU_HxV.f90"),
                           str(ROOT / "tests" / "fortran" / "probes_check.f90"),
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

    gs, sec = hxv.HxvSector.from_model(m, N, N), hxv.HxvSector.from_model(m, N + 1, N)
    e0, psi, _ = gs.lanczos_eigh(512, 1e-14, native=True)
    (v, n2v), (p, _) = gs.apply_ladder(sec, 0, 0, True, psi), gs.apply_ladder(sec, 1, 0, True, psi)
    a, b, ov, n = sec.lanczos_tridiag_probes(v, [p], 30)
    poles, w = greens.poles_weights(a[:n], b[:n], ov, np.sqrt(n2v))
    gs.close()
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    assert int(_floats(txt, "nsteps")[0]) == n == 30
    assert abs(_floats(txt, "E0")[0] - e0) < 1e-10 and abs(_floats(txt, "norm2")[0] - n2v) < 1e-10
    got_w = _floats(txt, "w_re") + 1j * _floats(txt, "w_im")
    # (the ground state comes back with the same global sign from the same deterministic start vector; a weight is bilinear in it anyway)
    assert np.abs(w).max() > 1e-3                                            # G_01 carries weight
    assert np.abs(_floats(txt, "poles") - poles).max() < 1e-10
    assert np.abs(got_w - w[:, 0]).max() < 1e-10
