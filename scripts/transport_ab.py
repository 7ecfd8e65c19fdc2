"""A/B of two builds of libhxv.so around a change of the rank transports or of the slab exchange (csrc/hxv_transport.cpp,
csrc/hxv_exchange.cpp): same bits, same counters, same speed.  One MI355X, thread ranks (RCCL's own transport cannot run two ranks on one
device); the RCCL branches run through tests/rccl_double (build it first: __graft_entry__.build_rccl_double()).

  HXV_LIB=<libhxv.so> python scripts/transport_ab.py run OUT.npz     every output below for every case, from ONE fresh process per library
  python scripts/transport_ab.py compare A.npz B.npz                 np.array_equal array by array (the counters are arrays too); exit 1 on a difference
  python scripts/transport_ab.py speed PARENT_LIB [NEW_LIB]          the three timing legs, parent and new alternating, three repetitions each,
                                                                     one fresh process per measurement; prints the table and the verdicts

Cases (the smallest shapes at which the paths differ), each under allgather, halo and alltoall and under both transports:
  chain_2, chain_3   hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6]) (3,3), DimDw 20, on 2 and on 3 ranks (3: uneven, one rank owns a column less)
  C2_4               hm_1dchain(eps_bath=[0.3, 0.6]) (6,6) on 4 ranks
  bhz_3              bhz_2d(Nbath=0) (4,4) on 3 ranks: complex H, no real-vector mode, no paired tridiagonalisation
Outputs per rank: the slab product from apply_device_slab, from slab_home() where the mode has one, and from apply_host; alpha and beta of
lanczos_tridiag (fused) from a complex and from a real start vector, and of lanczos_tridiag_pair; the eigenvalues of eigh_lowest; a split
twin_vector; the observables record, the cluster density matrix, a subset density matrix and apply_density_ops; one spin-dw ladder
operator into the sector with one more dw electron; exchange_count, slab_copies and allreduce_count after all of it.
speed: (a) bench.py plain, C3 ms_per_step; (b) scripts/exchange_modes_c3.py 4, ms per product of each mode -- engine-side work of thread
ranks sharing one GPU, not link time; (c) scripts/twin_split_bench.py at 4 ranks, split_ms.  Criterion: the new library's median over its
three repetitions lies within the parent's own range over its three, widened by that range once more on either side."""
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "cdmft-lanc-ed_amd")]
DOUBLE = ROOT / "tests" / "rccl_double" / "_build" / "librccl_double.so"
EXCHANGES = ("allgather", "halo", "alltoall")


def cases():
    from hxv import models

    chain = models.hm_1dchain(Nlat=2, Nbath=2, eps_bath=[0.3, 0.6])
    return [("chain_2", chain, (3, 3), 2, True), ("chain_3", chain, (3, 3), 3, True),
            ("C2_4", models.hm_1dchain(eps_bath=[0.3, 0.6]), (6, 6), 4, True), ("bhz_3", models.bhz_2d(Nbath=0), (4, 4), 3, False)]


def run_case(out, tag, m, nup, ndw, nranks, real_h, transport):
    import torch
    import hxv

    ser = hxv.HxvSector.from_model(m, nup, ndw)
    dim, nimp = ser.Dim, m.Nimp
    ser.close()
    rng = np.random.default_rng(5)
    vc = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    vc /= np.linalg.norm(vc)
    vr = rng.standard_normal(dim).astype(np.complex128)
    vr /= np.linalg.norm(vr)
    coef = rng.standard_normal((2, 2, nimp))
    exchange = tag.split("/")[1]

    def main(r, group):
        sec = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
        assert sec.exchange_mode == exchange
        group.join(sec)
        lo, hi = sec.mpiIshift, sec.mpiIshift + sec.vecDim
        slab = sec.pad(torch.from_numpy(vc[lo:hi].copy()).cuda(), sec.mpiQdw).contiguous().view(-1)
        res = {"slab": sec.apply_device_slab(slab).cpu().numpy(), "host": sec.apply_host(vc[lo:hi])}
        if exchange != "alltoall":
            home = sec.slab_home()
            home.copy_(slab)
            res["home"] = sec.apply_device_slab(home).cpu().numpy()
        for name, v in (("tri_c", vc), ("tri_r", vr)):
            a, b, n = sec.lanczos_tridiag(torch.from_numpy(v[lo:hi].copy()).cuda(), 25)
            res[name + "_alpha"], res[name + "_beta"], res[name + "_n"] = a, b, np.array(n)
        if real_h:
            (a0, b0, n0), (a1, b1, n1) = sec.lanczos_tridiag_pair(torch.from_numpy(vr[lo:hi].copy()).cuda(), torch.from_numpy(vr[lo:hi][::-1].copy()).cuda(), 25)
            res.update(pair_a0=a0, pair_b0=b0, pair_a1=a1, pair_b1=b1, pair_n=np.array([n0, n1]))
        ev, _, nc, nmv = sec.eigh_lowest(2, 16, 200, 0.0)
        res["eigh"], res["eigh_n"] = ev, np.array([nc, nmv])
        res["twin"] = sec.twin_vector(sec, slab).cpu().numpy()
        res["observables"] = sec.observables_record(slab, 0.7)
        if nimp <= 5:  # (no cluster density matrix beyond Nimp = 5)
            res["cluster_dm"] = sec.cluster_dm(slab, 0.7)
        res["subset_dm"] = sec.reduced_dm(slab, [0, nimp - 1], 0.7, fermi_sign=True)
        vecs, mean, nrm = sec.apply_density_ops(coef, slab)
        res.update(dop_mean=mean, dop_norm=nrm, **{f"dop_{i}": x.cpu().numpy() for i, x in enumerate(vecs)})
        res["counters"] = np.array([sec.exchange_count, sec.get_option("slab_copies"), sec.get_option("allreduce_count")], dtype=np.int64)
        sec.close()
        return res

    def ladder(r, group):
        fa = hxv.HxvSector.from_model(m, nup, ndw, rank=r, nranks=nranks)
        fb = hxv.HxvSector.from_model(m, nup, ndw + 1, rank=r, nranks=nranks)
        group.join(fb)
        slab = fa.pad(torch.from_numpy(vc[fa.mpiIshift: fa.mpiIshift + fa.vecDim].copy()).cuda(), fa.mpiQdw)
        o, nrm = fa.apply_ladder(fb, 1, 1, True, slab)
        res = {"ladder_dw": o.cpu().numpy(), "ladder_dw_norm": np.array(nrm)}
        fa.close()
        fb.close()
        return res

    for fn in (main, ladder):
        for r, res in enumerate(hxv.run_ranks(nranks, fn, transport=transport)):
            for k, x in res.items():
                out[f"{tag}/r{r}/{k}"] = np.asarray(x)


def run(path):
    import torch  # noqa: F401
    import hxv

    assert DOUBLE.exists(), f"{DOUBLE} is missing: build_rccl_double() first"
    os.environ["HXV_RCCL_LIB"] = str(DOUBLE)
    out = {}
    for name, m, (nup, ndw), nranks, real_h in cases():
        for exchange in EXCHANGES:
            hxv.set_exchange_default(exchange)
            try:
                for transport in ("local", "rccl"):
                    run_case(out, f"{name}/{exchange}/{transport}", m, nup, ndw, nranks, real_h, transport)
            finally:
                hxv.set_exchange_default("allgather")
    np.savez(path, **out)
    print(f"library {hxv.engine.LIB_PATH}: {len(out)} arrays in {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    same_keys = sorted(a.files) == sorted(b.files)
    by_what, bad = {}, []
    for k in sorted(set(a.files) & set(b.files)):
        ok = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True)
        what = k.rsplit("/", 1)[1]
        n, good = by_what.get(what, (0, 0))
        by_what[what] = (n + 1, good + ok)
        if not ok:
            bad.append(k)
    print(f"arrays: {len(a.files)} and {len(b.files)}, the same names: {same_keys}")
    for what, (n, good) in sorted(by_what.items()):
        print(f"  {what:16s} {good:4d} of {n:4d} bit-identical" + ("" if good == n else "   DIFFERENT"))
    nz = sum(int(np.count_nonzero(a[k])) for k in a.files)
    print(f"nonzero entries in all: {nz}; bit-identical: {sum(g for _, g in by_what.values())} of {sum(n for n, _ in by_what.values())}")
    for k in bad[:20]:
        print("  differs:", k)
    return 0 if same_keys and not bad else 1


# ---- speed ------------------------------------------------------------------------------------------------------------------------------
def _leg(cmd, lib, limit):
    """one fresh process with the library `lib`; -> its stdout.  A failure or a time limit ends the whole run: nothing more is started."""
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HXV_LIB=str(lib)), capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.exit(f"{' '.join(cmd)} with {lib}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout


def _measure(lib):
    py = sys.executable
    row = {}
    out = _leg([py, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "20"], lib, 600)
    row["bench C3 ms_per_step"] = json.loads(out.strip().splitlines()[-1])["ms_per_step"]
    out = _leg([py, "scripts/exchange_modes_c3.py", "4"], lib, 600)
    for mode, ms in re.findall(r"thread ranks, (\w+)\s*:\s*([0-9.]+) ms per product", out):
        row[f"exchange_modes_c3 4 ranks {mode} ms"] = float(ms)
    with tempfile.TemporaryDirectory() as tmp:  # (the script's own copy of its lines: not wanted here)
        out = _leg([py, "scripts/twin_split_bench.py", "--ranks", "4", "--no-host", "--out", str(Path(tmp) / "twin_split.json")], lib, 600)
    row["twin_split_bench 4 ranks split_ms"] = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]["split_ms"]
    return row


def speed(parent, new):
    rows = {"parent": [], "new": []}
    for rep in range(3):
        for who, lib in (("parent", parent), ("new", new)):
            rows[who].append(_measure(lib))
            print(f"-- {who} rep {rep + 1}: {json.dumps(rows[who][-1])}", flush=True)
    print(f"{'leg':44s} {'parent (3 reps)':28s} {'new (3 reps)':28s} {'new med':>9s}   allowed              verdict")
    worse = 0
    for leg in rows["parent"][0]:
        p, n = [r[leg] for r in rows["parent"]], [r[leg] for r in rows["new"]]
        lo, hi, med = min(p), max(p), float(np.median(n))
        a0, a1 = lo - (hi - lo), hi + (hi - lo)
        verdict = "inside" if a0 <= med <= a1 else "FASTER" if med < a0 else "SLOWER"
        worse += verdict == "SLOWER"
        print(f"{leg:44s} {' '.join(f'{x:8.4f}' for x in p):28s} {' '.join(f'{x:8.4f}' for x in n):28s} {med:9.4f}   [{a0:8.4f},{a1:8.4f}]  {verdict}")
    print(f"legs above the parent's widened range: {worse}")
    return 1 if worse else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) in (3, 4) and sys.argv[1] == "speed":
        sys.exit(speed(Path(sys.argv[2]).resolve(), Path(sys.argv[3] if len(sys.argv) == 4 else ROOT / "cdmft-lanc-ed_amd" / "lib" / "libhxv.so").resolve()))
    else:
        sys.exit(__doc__)
