"""The seeded random model generator of the parity sweeps (tests/test_gpu_fuzz.py, tests/test_gpu_row_order_sweep.py): random Hermitian
one-body matrices (spin-diagonal, as the N_up (x) N_dw path requires), random bath levels / hybridisations / interaction constants."""
import numpy as np


def random_model(rng, max_ns=9, min_bath=0, p_exchange=0.4):
    """A random model of at most `max_ns` orbitals per spin.  The defaults are tests/test_gpu_fuzz.py's generator as it always was (the
    same draws from `rng`, so a seed gives the fuzz the model it always had); the row-order sweep asks for larger models (`max_ns` 12, at
    least `min_bath` replicas where they fit) and Jx / Jp more often (each on with probability `p_exchange` when Norb > 1)."""
    from hxv.models import Model

    Nlat, Norb = [(1, 1), (2, 1), (3, 1), (2, 2), (1, 2), (4, 1), (1, 3)][rng.integers(7)]
    Nspin = int(rng.integers(1, 3))
    Nbath = int(rng.integers(min_bath, 3))
    while Nlat * Norb * (Nbath + 1) > max_ns:
        Nbath -= 1
    cplx = rng.random() < 0.5

    def herm_block():  # Hermitian in the (lat,orb) index, spin-diagonal
        n = Nlat * Norb
        A = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.6)
        if cplx:
            A = A + 1j * rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.4)
        A = (A + A.conj().T) / 2
        return A

    def to6(blocks):  # (Nlat,Nlat,Nspin,Nspin,Norb,Norb), index (ilat,iorb) -> iorb + ilat*Norb  (ED_SETUP.f90 imp_state_index)
        h = np.zeros((Nlat, Nlat, Nspin, Nspin, Norb, Norb), dtype=np.complex128)
        for s in range(Nspin):
            A = blocks[s]
            for il in range(Nlat):
                for jl in range(Nlat):
                    for io in range(Norb):
                        for jo in range(Norb):
                            h[il, jl, s, s, io, jo] = A[io + il * Norb, jo + jl * Norb]
        return h

    hloc = to6([herm_block() for _ in range(Nspin)])
    B = max(Nbath, 1)
    hb = np.zeros((Nlat, Nlat, Nspin, Nspin, Norb, Norb, B), dtype=np.complex128)
    vb = np.zeros((Nlat, Nspin, Norb, B))
    for ib in range(Nbath):
        hb[..., ib] = to6([herm_block() for _ in range(Nspin)])
        vb[..., ib] = rng.standard_normal((Nlat, Nspin, Norb)) * (rng.random((Nlat, Nspin, Norb)) < 0.8)
    U = np.zeros(5)
    U[:Norb] = rng.random(Norb) * 3
    multi = Norb > 1
    return Model(Nlat, Norb, Nspin, Nbath, hloc, hb[..., :B] if Nbath else hb[..., :0].reshape(Nlat, Nlat, Nspin, Nspin, Norb, Norb, 0),
                 vb[..., :B] if Nbath else vb[..., :0], Uloc=U, Ust=float(rng.random()) if multi else 0.0, Jh=float(rng.random() * 0.5) if multi else 0.0,
                 Jx=float(rng.random() * 0.4) if multi and rng.random() < p_exchange else 0.0, Jp=float(rng.random() * 0.4) if multi and rng.random() < p_exchange else 0.0,
                 xmu=float(rng.standard_normal() * 0.3), hfmode=bool(rng.integers(2)), name="fuzz")
