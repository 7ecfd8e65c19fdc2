"""The models and sectors on which the reference's own loop nests (oracle/ref_pin.f90, oracle/reference_pin.py) are run: shared by
tests/test_reference_pin.py (CPU, needs the binary) and scripts/make_golden_reference.py (writes tests/golden/reference_hxv.npz, which
tests/test_gpu_reference_parity.py reads without the binary).  Chosen so that every branch of the eight fragments runs: Nbath = 0 and > 0,
real and complex amplitudes, Norb 1 / 2 / 3, Nspin 1 / 2 (the `Nspin` spin index of H_dw), Jx alone, Jp alone, both, both hfmode values,
xmu != 0, non-zero bath diagonals, and the empty, full and one-particle sectors."""
import numpy as np

from random_models import random_model

KANAMORI = dict(Nx=2, Ny=1, Nbath=1, Ust=0.7, Jh=0.2)
RANDOM_SEED0 = 9000
SHAPES_WANTED = {(3, 1), (1, 3), (2, 2), (4, 1)}


def named_cases():
    """[(label, model, [(nup, ndw), ...])]"""
    from hxv import models

    return [
        ("chain", models.hm_1dchain(Nlat=2, Nbath=2), [(3, 3), (2, 4)]),
        ("chain_nohf_xmu", models.hm_1dchain(Nlat=2, Nbath=2, hfmode=False, xmu=0.3), [(3, 3)]),
        ("square", models.hm_2dsquare(Nbath=1), [(4, 3)]),
        ("plaquette", models.plaquette_2x2_nobath(), [(2, 2), (1, 3)]),
        ("plaquette_hf_xmu", models.plaquette_2x2_nobath(hfmode=True, xmu=0.1), [(2, 2)]),
        ("bhz_jx_jp", models.bhz_2d(Jx=0.2, Jp=0.15, **KANAMORI), [(4, 4), (3, 5)]),
        ("bhz_jx", models.bhz_2d(Jx=0.2, **KANAMORI), [(4, 4), (3, 5), (2, 6)]),
        ("bhz_jp", models.bhz_2d(Jp=0.15, **KANAMORI), [(4, 4), (3, 5), (2, 6)]),
        ("bhz_jx_jp_nohf_xmu", models.bhz_2d(Jx=0.2, Jp=0.15, hfmode=False, xmu=-0.2, **KANAMORI), [(3, 5)]),
    ]


def quirk_case():
    """Nlat > Norb, Nbath > 0, non-zero bath diagonal: direct/HxV_local.f90:83 drops the bath energies of the sites ilat > Norb"""
    from hxv import models

    return "chain_eps", models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, -0.2]), [(3, 3)]


def _edge_sectors(Ns):
    return [(0, 0), (Ns, Ns), (1, 0), (0, 1), (1, 1), (Ns - 1, Ns), (0, Ns), (1, Ns - 1)]


def random_cases():
    """random_model draws from seed RANDOM_SEED0 upwards, every draw taken, until there are at least twelve AND the shapes (Nlat,Norb) =
    (3,1), (1,3), (2,2), (4,1) and both Nspin values have come up.  Each draw: the sector nearest half filling and one of the edge sectors
    (empty, full, one particle, ...) in rotation."""
    out, shapes, nspins, k = [], set(), set(), 0
    while len(out) < 12 or not SHAPES_WANTED <= shapes or nspins != {1, 2}:
        assert k < 64, "the generator no longer produces the wanted shapes"
        m = random_model(np.random.default_rng(RANDOM_SEED0 + k))
        m.name = f"random{RANDOM_SEED0 + k}"
        Ns = m.Ns
        edges = _edge_sectors(Ns)
        out.append((m.name, m, [(Ns // 2, (Ns + 1) // 2), edges[k % len(edges)]]))
        shapes.add((m.Nlat, m.Norb))
        nspins.add(m.Nspin)
        k += 1
    return out


def all_cases():
    return named_cases() + [quirk_case()] + random_cases()


def flat_cases():
    """[(id, model, nup, ndw)]"""
    return [(f"{label}-{nup}-{ndw}", m, nup, ndw) for label, m, sectors in all_cases() for nup, ndw in sectors]


def dropped_bath_diagonal(model, map_up, map_dw):
    """What direct/HxV_local.f90:83-91 leaves out of the diagonal: its ilat loop ends at size(bath_diag,3) = Norb, so the bath energies
    bath_diag(ilat,1,iorb,ibath) n_up + bath_diag(ilat,Nspin,iorb,ibath) n_dw of the sites Norb < ilat <= Nlat never enter.  Returned as the
    diagonal (length Dim, i = iup + (idw-1) DimUp); zero whenever Nlat <= Norb, Nbath = 0 or those bath levels vanish."""
    L, O, S, B = model.Nlat, model.Norb, model.Nspin, model.Nbath
    mu, md = np.asarray(map_up, dtype=np.int64), np.asarray(map_dw, dtype=np.int64)
    d_up, d_dw = np.zeros(mu.size), np.zeros(md.size)
    for il in range(O, L):                    # 0-based sites Norb .. Nlat-1
        for io in range(O):
            for ib in range(B):
                bit = L * O * (ib + 1) + io + il * O          # getBathStride - 1
                d_up += model.Hbath[il, il, 0, 0, io, io, ib].real * ((mu >> bit) & 1)
                d_dw += model.Hbath[il, il, S - 1, S - 1, io, io, ib].real * ((md >> bit) & 1)
    return (d_up[:, None] + d_dw[None, :]).reshape(-1, order="F")


# ---- the recorded subset (tests/golden/reference_hxv.npz): every sector has 3 <= DimDw, Dim <= 4900 ----
GOLDEN_IDS = ["chain-3-3", "chain-2-4", "chain_nohf_xmu-3-3", "square-4-3", "plaquette-2-2", "bhz_jx_jp-3-5", "bhz_jx-2-6", "bhz_jp-2-6",
              "chain_eps-3-3"]
GOLDEN_RANDOM = 4      # + the near-half-filling sector of the first draws that fit, one of them with Nlat < Norb and a bath if there is one


def golden_cases():
    flat = {cid: (m, nup, ndw) for cid, m, nup, ndw in flat_cases()}
    out = [(cid,) + flat[cid] for cid in GOLDEN_IDS]
    from math import comb

    picked, have_excluded = 0, False
    for label, m, sectors in random_cases():
        excluded = m.Nbath > 0 and m.Nlat < m.Norb
        if picked >= GOLDEN_RANDOM and not (excluded and not have_excluded):
            continue
        for nup, ndw in (sectors[0], (2, m.Ns - 2)):      # (the second: small enough at Ns = 9)
            if comb(m.Ns, ndw) >= 3 and comb(m.Ns, nup) >= 3 and comb(m.Ns, nup) * comb(m.Ns, ndw) <= 1300:
                out.append((f"{label}-{nup}-{ndw}", m, nup, ndw))
                picked += 1
                have_excluded = have_excluded or excluded
                break
    return out
