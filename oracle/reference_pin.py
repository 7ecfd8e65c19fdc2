"""The reference's OWN Hamiltonian loop nests, executed (oracle/ref_pin.f90).  TEST INFRASTRUCTURE ONLY.

The reference's modules cannot be built here (SciFortran, MPI, revision.inc: DESIGN.md section 1), but its hot path is kept as include
fragments without a USE line: ED_HAMILTONIAN/sparse/{H_local,H_non_local,H_up,H_dw}.f90 (the matrix build behind spMatVec_main) and
ED_HAMILTONIAN/direct/{HxV_local,HxV_up,HxV_dw,HxV_non_local}.f90 (the same operator applied on the fly).  oracle/ref_pin.f90 declares
the scope they expect and includes them at compile time; build_reference() is the recipe, the binary lands in oracle/_ref/ (ignored by
git: it is compiled from reference text).  Where the reference tree is absent the binary that is already there is kept.

run(model, nup, ndw, vin) -> the four element streams in insertion order and, where it may run, Hv of directMatVec_main's body.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
SRC = _HERE / "ref_pin.f90"
OUT_DIR = _HERE / "_ref"
BIN = OUT_DIR / "ref_pin"
FRAGMENTS = [f"ED_HAMILTONIAN/sparse/{n}.f90" for n in ("H_local", "H_non_local", "H_up", "H_dw")] + \
            [f"ED_HAMILTONIAN/direct/{n}.f90" for n in ("HxV_local", "HxV_up", "HxV_dw", "HxV_non_local")]
STREAM_IDS = {"d": 1, "nd": 2, "up": 3, "dw": 4}      # spH0d, spH0nd, spH0ups(1), spH0dws(1)
_REC = np.dtype([("id", "<i4"), ("i", "<i4"), ("j", "<i4"), ("re", "<f8"), ("im", "<f8")])


def reference_tree() -> Path | None:
    """the reference checkout: $HXV_REFERENCE_DIR, else a directory `reference` beside the repository, else /root/reference (where SURVEY.md
    and the citations of hxv_oracle.c read it); None when its fragments are nowhere"""
    env = os.environ.get("HXV_REFERENCE_DIR")
    for d in ([Path(env)] if env else []) + [_HERE.parent.parent / "reference", Path("/root/reference")]:
        try:
            if all((d / f).is_file() for f in FRAGMENTS):
                return d
        except OSError:      # (a directory this user may not read)
            pass
    return None


def build_reference(force: bool = False) -> Path | None:
    """oracle/_ref/ref_pin from oracle/ref_pin.f90 and the reference's fragments (flang, as the Fortran glue).  Without the reference tree
    or without flang: whatever binary is already there (None if none) -- never an error."""
    flang = os.environ.get("FLANG", "/opt/rocm/lib/llvm/bin/flang")
    tree = reference_tree()
    if tree is None or not Path(flang).exists():
        return BIN if BIN.exists() else None
    deps = [SRC] + [tree / f for f in FRAGMENTS]
    if force or not BIN.exists() or any(p.stat().st_mtime > BIN.stat().st_mtime for p in deps):
        OUT_DIR.mkdir(parents=True, exist_ok=True)
        # -ffp-contract=off: the streams are compared bit for bit with the C oracle, which is built without contraction too
        subprocess.check_call([flang, "-O2", "-ffp-contract=off", f"-I{tree}", "-J", str(OUT_DIR), "-o", str(BIN), str(SRC)])
    return BIN


def available() -> bool:
    return build_reference() is not None


def sector_map(Ns: int, n: int) -> np.ndarray:
    """the states of Ns orbitals with n particles, ascending (ours; the reference's build_sector is not executed)"""
    s = np.arange(1 << Ns, dtype=np.int64)
    pop = np.zeros_like(s)
    for b in range(Ns):
        pop += (s >> b) & 1
    return s[pop == n].astype(np.int32)


def write_input(path, model, nup: int, ndw: int, vin: np.ndarray):
    mu, md = sector_map(model.Ns, nup), sector_map(model.Ns, ndw)
    vin = np.ascontiguousarray(vin, dtype=np.complex128)
    assert vin.size == mu.size * md.size
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", model.Nlat, model.Norb, model.Nspin, model.Nbath, int(bool(model.hfmode)), nup, ndw, mu.size, md.size))
        f.write(struct.pack("<10d", *[float(u) for u in model.Uloc[:5]], float(model.Ust), float(model.Jh), float(model.Jx), float(model.Jp), float(model.xmu)))
        f.write(np.ascontiguousarray(model.impHloc.ravel(order="F"), dtype=np.complex128).tobytes())
        if model.Nbath > 0:
            f.write(np.ascontiguousarray(model.Hbath.ravel(order="F"), dtype=np.complex128).tobytes())
            f.write(np.ascontiguousarray(model.Vbath.ravel(order="F"), dtype=np.float64).tobytes())
        f.write(mu.tobytes())
        f.write(md.tobytes())
        f.write(vin.tobytes())
    return mu, md


def direct_runs(model) -> bool:
    """direct/HxV_local.f90:83 bounds its ilat bath loop by size(bath_diag,3) = Norb: with Nlat < Norb and a bath it indexes past bath_diag"""
    return not (model.Nbath > 0 and model.Nlat < model.Norb)


class ReferenceRun:
    """what the reference's loops produced for one (model, sector, vin)"""

    def __init__(self, model, nup, ndw, map_up, map_dw, records, hv):
        self.model, self.nup, self.ndw = model, nup, ndw
        self.map_up, self.map_dw = map_up, map_dw
        self.DimUp, self.DimDw = map_up.size, map_dw.size
        self.Dim = self.DimUp * self.DimDw
        self.records = records
        self.hv = hv                                  # output B, None where the direct fragments may not run

    def stream(self, which: str):
        """(i, j, values) of one matrix in call order; i, j 1-based as the fragments passed them"""
        r = self.records[self.records["id"] == STREAM_IDS[which]]
        return r["i"].astype(np.int64), r["j"].astype(np.int64), r["re"] + 1j * r["im"]

    def csr(self, which: str):
        """the stream stored the way ED_SPARSE_MATRIX.f90:267-273 stores it -> (rowptr int64, cols int32 1-based, vals), OracleSector.csr's form"""
        n = {"up": self.DimUp, "dw": self.DimDw, "nd": self.Dim, "d": self.Dim}[which]
        return stream_to_csr(*self.stream(which), n)

    def diag(self):
        rp, cols, vals = self.csr("d")
        assert np.array_equal(rp, np.arange(self.Dim + 1)) and np.array_equal(cols, np.arange(1, self.Dim + 1)), "spH0d: one (i,i) element per row"
        return vals

    def matrices(self):
        import scipy.sparse as sp

        out = {}
        for which, n in (("up", self.DimUp), ("dw", self.DimDw), ("nd", self.Dim)):
            rp, cols, vals = self.csr(which)
            out[which] = sp.csr_matrix((vals, cols.astype(np.int64) - 1, rp), shape=(n, n))
        return out

    def full_matrix(self):
        """spH0d + 1 (x) H_up + H_dw (x) 1 + spH0nd, i = iup + (idw-1) DimUp (ED_HAMILTONIAN_SPARSE_HxV.f90:112-148)"""
        import scipy.sparse as sp

        m = self.matrices()
        return (sp.diags(self.diag()) + sp.kron(m["dw"], sp.identity(self.DimUp)) + sp.kron(sp.identity(self.DimDw), m["up"]) + m["nd"]).tocsr()

    def stream_product(self, v):
        return self.full_matrix() @ np.asarray(v, dtype=np.complex128)


def stream_to_csr(i, j, vals, nrows):
    """Row lists in insertion order; a repeated (i,j) is summed where it first stands, in call order."""
    i, j, vals = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(vals, dtype=np.complex128).copy()
    keep = np.ones(i.size, dtype=bool)
    if i.size:
        key = i * (int(j.max()) + 1) + j
        _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
        if first.size != i.size:
            for k in np.flatnonzero(first[inverse] != np.arange(i.size)):      # repeated elements, in call order
                vals[first[inverse[k]]] += vals[k]
                keep[k] = False
    i, j, vals = i[keep], j[keep], vals[keep]
    order = np.argsort(i, kind="stable")
    rp = np.zeros(nrows + 1, dtype=np.int64)
    np.add.at(rp, i, 1)
    return np.cumsum(rp), j[order].astype(np.int32), vals[order]


def run(model, nup: int, ndw: int, vin: np.ndarray, direct: bool | None = None) -> ReferenceRun:
    exe = build_reference()
    if exe is None:
        raise RuntimeError("no reference tree and no built oracle/_ref/ref_pin")
    if direct is None:
        direct = direct_runs(model)
    if direct and not direct_runs(model):
        raise ValueError("the direct fragment indexes past bath_diag for Nlat < Norb with a bath: never run")
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        mu, md = write_input(d / "in.bin", model, nup, ndw, vin)
        cmd = [str(exe), str(d / "in.bin"), str(d / "streams.bin")] + ([str(d / "hv.bin")] if direct else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"ref_pin failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-500:]}")
        records = np.fromfile(d / "streams.bin", dtype=_REC)
        hv = np.fromfile(d / "hv.bin", dtype=np.complex128) if direct else None
    return ReferenceRun(model, nup, ndw, mu, md, records, hv)
