"""Paired probe runs through the Fortran glue (gpu_sp_lanc_tridiag_pair_probes_dev; fortran/ED_HAMILTONIAN_GPU_HxV.f90): a small flang host
(tests/fortran/pair_probes_check.f90, built by build_pair_probes_check) uploads two real start vectors and three real probes of the Ns = 6
chain's sector (4,3), written by this test, runs ONE paired tridiagonalisation and prints alanc, blanc and the real overlaps of both runs with
every digit; they are the Python route's numbers, bit for bit, and no sector is left open."""
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NLANC = 30


def _floats(txt, key):
    return np.array([float(x) for x in re.search(rf"^{key}=\s*(.*)$", txt, re.M).group(1).split()])


def test_fortran_glue_pair_probes_equal_the_python_path(built, tmp_path):
    import hxv
    from hxv import models

    exe = built.build_pair_probes_check()
    if exe is None:
        pytest.skip("flang not available")
    m, (nup, ndw), nprobes = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.25, -0.4], U=2.0), (4, 3), 3      # DimUp = 15: pad rows
    sec = hxv.HxvSector.from_model(m, nup, ndw)
    rng = np.random.default_rng(12)
    vecs = [rng.standard_normal(sec.Dim).astype(np.complex128) for _ in range(2 + nprobes)]
    vecs[1] *= 0.3                                                                # (start vectors need not be normalised)
    inp = tmp_path / "model.bin"
    with open(inp, "wb") as f:
        np.array([m.Nlat, m.Norb, m.Nspin, m.Nbath, nup, ndw, int(m.hfmode)], dtype=np.int32).tofile(f)
        m.impHloc.ravel(order="F").tofile(f)
        m.Hbath.ravel(order="F").tofile(f)
        m.Vbath.ravel(order="F").tofile(f)
        np.concatenate([m.Uloc, [m.Ust, m.Jh, m.Jx, m.Jp, m.xmu]]).astype(np.float64).tofile(f)
        np.array([nprobes, sec.Dim], dtype=np.int32).tofile(f)
        for v in vecs:
            v.tofile(f)
    out = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    txt = out.stdout

    dev = [sec.vector_from_host(v) for v in vecs]
    runs = sec.lanczos_tridiag_pair_probes(dev[0], dev[1], dev[2:], NLANC)
    sec.close()
    assert int(_floats(txt, "live_sectors")[0]) == 0
    for x, (a, b, ov, n) in zip("ab", runs):
        assert int(_floats(txt, f"nsteps_{x}")[0]) == n == NLANC
        assert np.array_equal(_floats(txt, f"alanc_{x}"), a) and np.array_equal(_floats(txt, f"blanc_{x}"), b)
        assert not ov.imag.any() and np.abs(ov).max() > 1e-3
        for j in range(nprobes):
            assert np.array_equal(_floats(txt, f"ov_{x}{j + 1}"), ov[:, j].real), (x, j)
