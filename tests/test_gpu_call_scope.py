"""A driver call leaves the device-buffer cache where it found it, however it returns (csrc/hxv_call_scope.hpp), and the table store of a
sector image keeps the last few table sets of a family (csrc/hxv_handle.hpp: TableStore).

The balance is read from hxv_get_option(h, "pool_live_blocks"): the blocks pool_alloc has handed out on the handle's device and that have
not come back.  Every entry that borrows per-call scratch is called once to warm what the HANDLE keeps (the Lanczos vectors, the dw-hop
scratch, the staging of the host entries); a second call must then leave the count exactly where it was, and so must a call that fails
after it has taken its scratch -- with the documented status, and with the next good call giving the bits of the one before the failure.
Failures that arguments can reach behind the scratch: an all-zero state (hxv_apply_density_ops, hxv_lanczos_tridiag[_probes]), ncv > 64
under hxv_eigh_lowest_host (hxv_eigh_lowest itself refuses it in front of its scratch), and on a split sector one rank's NULL list entry,
which reaches the peers -- scratch in hand -- through the agreement.  The other entries have no failure that arguments reach behind their
scratch; they take the normal-call half only.

Shapes: hm_1dchain(Nlat 2, Nbath 3), Ns = 8, sector (4,4), 70 x 70, with a device row order forced on (the hooks of
tests/test_gpu_twin.py: without one hxv_vector_from_host / _to_host take no scratch); its neighbours (3,4), (4,5) for the ladder, (3,3),
(5,5), (3,5), (5,3) for the spin pair, the twin pair (3,5) -> (5,3); bhz_2d(2 x 1, no bath), Nimp = 4, sector (2,2), for the four-orbital
mask.  Unsplit, and on 3 thread ranks (hxv_comm_init_local): the pool is per device and shared by the ranks, so the count is read by the main
thread only while every rank thread of a phase has been joined."""
import ctypes as C
import gc
import re
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ARG, HIP, STATE, UNSUPPORTED = 1, 2, 3, 4
NLANC = 12            # >= 8: the unsplit run without probes takes the device-only path and its alpha/beta arrays
MIN_DIMUP, ROW_BITS = 16, 4


def _chain():
    from hxv import models

    return models.hm_1dchain(Nlat=2, Nbath=3, eps_bath=[0.3, -0.2, 0.1], xmu=0.15)


def _two_orbital():
    from hxv import models

    return models.bhz_2d(Nx=2, Ny=1, Nbath=0, Ust=0.5, Jh=0.2)   # Nlat 2 x Norb 2: Nimp = Ns = 4


def _bits(x):
    """every number of a result (nested tuples / lists of tensors, arrays and scalars) as bytes"""
    import torch

    if isinstance(x, (tuple, list)):
        return b"|".join(_bits(y) for y in x)
    if torch.is_tensor(x):
        return torch.view_as_real(x).contiguous().cpu().numpy().tobytes() if x.is_complex() else x.cpu().numpy().tobytes()
    return np.ascontiguousarray(x).tobytes()


def _status(fn):
    """the status of a refused call made through the Python form"""
    import hxv

    with pytest.raises(hxv.HxvError) as ei:
        fn()
    return int(re.search(r"status (\d+)", str(ei.value)).group(1))


class _Rank:
    pass


class _Rig:
    """the sectors and vectors of every rank, kept open across phases; phase(fn) runs fn(rank state) on one fresh thread per rank and joins them"""

    def __init__(self, nranks):
        import hxv

        self.nranks = nranks
        self.groups = [hxv.LocalGroup(nranks) for _ in range(5)] if nranks > 1 else []   # (a group takes one handle per rank)
        self.ranks = [_Rank() for _ in range(nranks)]
        for r, k in enumerate(self.ranks):
            k.r, k.secs = r, []
        self.phase(self._open)

    def phase(self, fn):
        if not self.groups:
            return [fn(self.ranks[0])]
        out, err = [None] * self.nranks, []

        def work(k):
            try:
                out[k.r] = fn(k)
            except BaseException as e:  # noqa: BLE001 (re-raised below; the peers are woken instead of left in a collective)
                err.append(e)
                for g in self.groups:
                    g.abort()

        ts = [threading.Thread(target=work, args=(k,)) for k in self.ranks]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if err:
            raise err[0]
        return out

    def _open(self, k):
        import torch
        import hxv

        kw = dict(rank=k.r, nranks=self.nranks)
        m, m2 = _chain(), _two_orbital()

        def sector(model, nup, ndw, group=None):
            s = hxv.HxvSector.from_model(model, nup, ndw, **kw)
            k.secs.append(s)
            if group is not None and self.groups:
                self.groups[group].join(s)                         # (collective: the same order on every rank)
            return s

        k.s44, k.s34, k.s45 = sector(m, 4, 4, 0), sector(m, 3, 4, 1), sector(m, 4, 5, 2)
        k.s35, k.s53 = sector(m, 3, 5), sector(m, 5, 3, 3)
        k.two = sector(m2, 2, 2, 4)
        if self.nranks == 1:
            k.s33 = sector(m, 3, 3)
        assert k.s44.row_perm is not None                          # (the host copies go through their scratch)
        rng = np.random.default_rng(11)

        def slab(s, real=True):
            v = rng.standard_normal(s.Dim) + (0.0 if real else 1j * rng.standard_normal(s.Dim))
            v = (v / np.linalg.norm(v)).astype(np.complex128)
            return v[s.mpiIshift: s.mpiIshift + s.vecDim].copy()

        k.host = slab(k.s44)
        k.psi, k.p1, k.p2 = (k.s44.vector_from_host(h) for h in (k.host, slab(k.s44), slab(k.s44)))
        k.psi35 = k.s35.vector_from_host(slab(k.s35, real=False))
        k.psi2 = k.two.vector_from_host(slab(k.two, real=False))
        if self.nranks == 1:
            k.psi33 = k.s33.vector_from_host(slab(k.s33))
        k.zero = torch.zeros_like(k.psi)
        k.cf = np.random.default_rng(6).standard_normal((2, 2, 2))
        torch.cuda.synchronize()

    def live(self):
        return self.ranks[0].s44.get_option("pool_live_blocks")

    def close(self):
        def shut(k):
            for s in k.secs:
                s.close()

        try:
            self.phase(shut)
        finally:
            for g in self.groups:
                g.close()


@pytest.fixture(scope="module")
def rigs(built):
    """-> get(nranks): the rig of that many ranks, opened on first use and kept for the module"""
    import hxv

    mp = pytest.MonkeyPatch()
    mp.setenv("HXV_LOCAL_TIMEOUT_S", "30")
    mp.setenv("HXV_ROW_ORDER_MIN_DIMUP", str(MIN_DIMUP))
    mp.setenv("HXV_ROW_ORDER_BITS", str(ROW_BITS))
    mp.delenv("HXV_ROW_ORDER", raising=False)
    hxv.sector_cache_clear()
    gc.collect()                                                   # (no sector of an earlier module is destroyed while a count is compared)
    made = {}

    def get(nranks):
        if nranks not in made:
            made[nranks] = _Rig(nranks)
        return made[nranks]

    try:
        yield get
    finally:
        for rig in made.values():
            rig.close()
        mp.undo()
        hxv.sector_cache_clear()


def _probes_direct(k, vin, null_on_rank):
    """hxv_lanczos_tridiag_probes through the C-ABI with two probes, the second one NULL on one rank -> status"""
    import torch
    import hxv

    pd = C.POINTER(C.c_double)
    a, b, ov, n = np.zeros(NLANC), np.zeros(NLANC), np.zeros(2 * NLANC * 2), C.c_int32()
    plist = (C.c_void_p * 2)(k.p1.data_ptr(), None if k.r == null_on_rank else k.p2.data_ptr())
    torch.cuda.synchronize()
    return hxv.load_library().hxv_lanczos_tridiag_probes(k.s44._h, vin.data_ptr(), 2, plist, NLANC, a.ctypes.data_as(pd), b.ctypes.data_as(pd),
                                                         ov.ctypes.data_as(pd), 1e-12, C.byref(n))


def _density_null(k):
    import torch

    outs = [torch.empty_like(k.psi) for _ in range(2)]
    return _status(lambda: k.s44.apply_density_ops(k.cf, k.psi, out=[outs[0], None if k.r == 0 else outs[1]]))


def _roundtrip(k):
    d = k.s44.vector_from_host(k.host)
    return d, k.s44.vector_to_host(d)


# entry -> (the good call, [(what fails, the call -> status, the statuses a rank may get: its own error / what the agreement hands a peer)])
OWN, PEER = (ARG,), (ARG, STATE)
ENTRIES = {
    "observables": (lambda k: k.s44.observables_record(k.psi), []),
    "cluster_dm": (lambda k: k.s44.cluster_dm(k.psi), []),
    "reduced_dm": (lambda k: k.two.reduced_dm(k.psi2, [0, 1, 2, 3]), []),
    "density_ops": (lambda k: k.s44.apply_density_ops(k.cf, k.psi),
                    [("an all-zero state", lambda k: _status(lambda: k.s44.apply_density_ops(k.cf, k.zero)), lambda k: OWN),
                     ("split: a NULL output entry on rank 0", _density_null, lambda k: OWN if k.r == 0 else PEER)]),
    "spin_pair": (lambda k: k.s33.apply_spin_pair(k.s44, [(0, 1, 1.0), (1, 0, 0.5)], True, True, k.psi33), []),
    "twin": (lambda k: k.s35.twin_vector(k.s53, k.psi35), []),
    "ladder_dw": (lambda k: k.s44.apply_ladder(k.s45, 2, 1, True, k.psi), []),
    "ladder_up": (lambda k: k.s44.apply_ladder(k.s34, 1, 0, False, k.psi), []),
    "tridiag": (lambda k: k.s44.lanczos_tridiag(k.psi, NLANC),
                [("an all-zero start vector", lambda k: _status(lambda: k.s44.lanczos_tridiag(k.zero, NLANC)), lambda k: OWN)]),
    "tridiag_probes": (lambda k: k.s44.lanczos_tridiag_probes(k.psi, [k.p1, k.p2], NLANC),
                       [("an all-zero start vector", lambda k: _status(lambda: k.s44.lanczos_tridiag_probes(k.zero, [k.p1, k.p2], NLANC)), lambda k: OWN),
                        ("split: a NULL probe on rank 0", lambda k: _probes_direct(k, k.psi, 0), lambda k: OWN if k.r == 0 else PEER)]),
    "lanczos_eigh": (lambda k: k.s44.lanczos_eigh(300, 1e-13, native=True), []),
    "eigh_lowest": (lambda k: k.s44.eigh_lowest(2, 16, 200, 0.0, native=True),
                    [("ncv > 64", lambda k: _status(lambda: k.s44.eigh_lowest(2, 65, 200, 0.0)), lambda k: OWN)]),
    "eigh_lowest_host": (lambda k: k.s44.eigh_lowest_host(2, 16, 200, 0.0),
                         [("ncv > 64", lambda k: _status(lambda: k.s44.eigh_lowest_host(2, 65, 200, 0.0)), lambda k: OWN)]),
    "vector_from_to_host": (_roundtrip, []),
}
CASES = [(n, e) for n in (1, 3) for e in ENTRIES if not (n == 3 and e == "spin_pair")]   # (hxv_apply_spin_pair refuses split sectors)


@pytest.mark.parametrize("nranks,entry", CASES, ids=[f"{n}rank-{e}" for n, e in CASES])
def test_a_driver_call_returns_every_block_it_took(rigs, nranks, entry):
    rig = rigs(nranks)
    good, failures = ENTRIES[entry]
    call = lambda k: _bits(good(k))  # noqa: E731
    rig.phase(call)                                               # warms what the handle keeps
    live0 = rig.live()
    first = rig.phase(call)
    live1 = rig.live()
    print(f"{entry} on {nranks} rank(s): pool_live_blocks {live0} -> {live1} over a normal call")
    assert live1 == live0, (entry, live0, live1)
    for what, fail, allowed in failures:
        if what.startswith("split") and nranks == 1:
            continue
        got = rig.phase(fail)
        live2 = rig.live()
        print(f"  {what}: status {got}, pool_live_blocks {live2}")
        for k, rc in zip(rig.ranks, got):
            assert rc in allowed(k), (entry, what, k.r, rc)
        assert live2 == live0, (entry, what, live0, live2)
        assert rig.phase(call) == first, (entry, what)            # the same bits as before the failure
        assert rig.live() == live0, (entry, what)


def test_the_table_store_keeps_the_last_eight_of_a_family(built, monkeypatch):
    """ten subset masks on one image: the first one has been dropped and builds again -- the same bits, no handle lost; then the spin pair
    into one target from every (source sector, source row order) the chain offers, nine at the most"""
    import torch
    import hxv

    for kenv in ("HXV_ROW_ORDER", "HXV_ROW_ORDER_MIN_DIMUP", "HXV_ROW_ORDER_BITS"):
        monkeypatch.delenv(kenv, raising=False)
    hxv.sector_cache_clear()
    gc.collect()
    live_handles0 = hxv.live_handles()
    two = hxv.HxvSector.from_model(_two_orbital(), 2, 2)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(two.Dim) + 1j * rng.standard_normal(two.Dim)
    psi = two.vector_from_host(v / np.linalg.norm(v))
    masks = [[0], [1], [2], [3], [0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    handles1, live1 = hxv.live_handles(), two.get_option("pool_live_blocks")
    first = [_bits(two.reduced_dm(psi, mk, fermi_sign=True)) for mk in masks]
    assert len(set(first)) == len(masks)
    again = _bits(two.reduced_dm(psi, masks[0], fermi_sign=True))          # (nine others since: its tables are built anew)
    assert again == first[0]
    assert _bits(two.reduced_dm(psi, masks[-1], fermi_sign=True)) == first[-1]     # ... and a kept one is served as it was
    assert hxv.live_handles() == handles1 and two.get_option("pool_live_blocks") == live1
    two.close()

    # spin pair into (4,4): a table set per (source sector, its row order, flags); the flags follow from the source
    m = _chain()
    to = hxv.HxvSector.from_model(m, 4, 4)
    sources, seen = [], set()
    for bits in (None, 4, 5, 3, 6, 2):
        if bits is None:
            monkeypatch.setenv("HXV_ROW_ORDER", "0")
        else:
            monkeypatch.delenv("HXV_ROW_ORDER", raising=False)
            monkeypatch.setenv("HXV_ROW_ORDER_MIN_DIMUP", str(MIN_DIMUP))
            monkeypatch.setenv("HXV_ROW_ORDER_BITS", str(bits))
        for nup, ndw in ((3, 3), (5, 5), (3, 5), (5, 3)):
            s = hxv.HxvSector.from_model(m, nup, ndw)
            key = (nup, ndw, None if s.row_perm is None else s.row_perm.tobytes())
            if key in seen or len(sources) == 9:
                s.close()
                continue
            seen.add(key)
            sources.append((s, nup < 4, ndw < 4))
    reached = len(sources)
    print(f"spin pair into (4,4): {reached} (source, row order, flags) combinations reached")
    assert reached >= 4                                                     # (the four source sectors; more than eight only where the orders exist)
    results = []
    for s, cup, cdw in sources:
        w = rng.standard_normal(s.Dim)
        dpsi = s.vector_from_host((w / np.linalg.norm(w)).astype(np.complex128))
        run = lambda s=s, cup=cup, cdw=cdw, dpsi=dpsi: _bits(s.apply_spin_pair(to, [(0, 1, 1.0), (1, 0, 0.5)], cup, cdw, dpsi))  # noqa: E731
        results.append((run, run()))
    for run, bits0 in results:                                              # the first one first: with nine it has been dropped meanwhile
        assert run() == bits0
    torch.cuda.synchronize()
    for s in [s for s, _, _ in sources] + [to]:
        s.close()
    assert hxv.live_handles() == live_handles0
