#!/usr/bin/env python3
"""Generate tests/golden/reference_hxv.npz: Hv as the REFERENCE'S OWN loop nests produced it (oracle/ref_pin.f90 -> oracle/_ref/ref_pin,
BUILD CONTAINER ONLY: needs the reference tree or a built binary; CPU, under a minute; nothing of the engine or of the C oracle is used).

For every case of tests/reference_cases.golden_cases() the file holds the settings the reference program read (the model's scalars and
arrays in the layout of hxv_model, the sector) and what it wrote: Hv of directMatVec_main's body on models.deterministic_vector(Dim)
(not stored).  Where the direct fragments may not run (Nlat < Norb with a bath) or drop the bath energies of the sites ilat > Norb
(direct/HxV_local.f90:83), Hv is the product of the reference's element streams instead (`source` 1).  One ground
state energy per model: numpy.linalg.eigvalsh of the dense matrix of the reference's streams, in the first stored sector of the model.

  python scripts/make_golden_reference.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "cdmft-lanc-ed_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from hxv import models  # noqa: E402  (operator INPUTS only)
from oracle import reference_pin as rp  # noqa: E402
import reference_cases as rc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "reference_hxv.npz"


def build_arrays(energy_max_dim=None):
    """name -> array, as stored.  energy_max_dim: leave e0 NaN for sectors larger than this (the regeneration test skips the two big ones)."""
    cases = rc.golden_cases()
    out = {"ids": np.array([c[0] for c in cases])}
    ints, reals, source, e0 = [], [], [], []
    seen_models = set()
    for k, (cid, m, nup, ndw) in enumerate(cases):
        v = models.deterministic_vector(len(rp.sector_map(m.Ns, nup)) * len(rp.sector_map(m.Ns, ndw)))
        ref = rp.run(m, nup, ndw, v)
        assert ref.Dim <= 4900 and ref.DimDw >= 3 and ref.DimUp >= 3, cid
        direct_ok = ref.hv is not None and not rc.dropped_bath_diagonal(m, ref.map_up, ref.map_dw).any()
        ints.append([m.Nlat, m.Norb, m.Nspin, m.Nbath, int(bool(m.hfmode)), nup, ndw])
        reals.append([float(u) for u in m.Uloc[:5]] + [float(m.Ust), float(m.Jh), float(m.Jx), float(m.Jp), float(m.xmu)])
        source.append(0 if direct_ok else 1)
        out[f"imphloc_{k}"] = np.ascontiguousarray(m.impHloc.ravel(order="F"))
        out[f"hbath_{k}"] = np.ascontiguousarray(m.Hbath.ravel(order="F"))
        out[f"vbath_{k}"] = np.ascontiguousarray(m.Vbath.ravel(order="F"))
        out[f"hv_{k}"] = ref.hv if direct_ok else ref.stream_product(v)
        label = cid.rsplit("-", 2)[0]
        if label in seen_models or (energy_max_dim is not None and ref.Dim > energy_max_dim):
            e0.append(np.nan)
        else:
            H = ref.full_matrix().toarray()
            assert np.abs(H - H.conj().T).max() == 0.0, cid
            e0.append(float(np.linalg.eigvalsh(H if H.imag.any() else np.ascontiguousarray(H.real))[0]))
        seen_models.add(label)     # (the model's first stored sector carries its energy)
        print(f"{cid:24s} Dim {ref.Dim:5d} source {'streams' if source[-1] else 'direct '} E0 {e0[-1]}", flush=True)
    out["ints"] = np.array(ints, dtype=np.int32)
    out["reals"] = np.array(reals, dtype=np.float64)
    out["source"] = np.array(source, dtype=np.int32)
    out["e0"] = np.array(e0, dtype=np.float64)
    return out


def main():
    if not rp.available():
        raise SystemExit("neither the reference tree nor a built oracle/_ref/ref_pin")
    arrays = build_arrays()
    np.savez_compressed(OUT, **arrays)
    size = OUT.stat().st_size
    print(f"wrote {OUT.relative_to(ROOT)}: {len(arrays['ids'])} cases, {size} bytes")
    assert size < 256 * 1024, size


if __name__ == "__main__":
    main()
