"""The twin-sector map in numpy, as the reference defines it (ED_SETUP.f90:854-898 twin_sector_order, ED_EIGENSPACE.f90:485-494
es_return_cvector): every state |up>|dw> of sector A = (nup,ndw) is flipped into |dw>|up>, a state of B = (ndw,nup); the flipped Fock numbers,
taken in A's index order, are sorted, and the sorting permutation is Order: v_B(i) = v_A(Order(i)).  No sign.  What include/hxv.h's
hxv_twin_vector does on the device, for tests on the CPU and on the GPU."""
import numpy as np


def twin_order(map_up, map_dw, ns):
    """Order (0-based) from the two sector maps of A (the Fock numbers of its up / dw configurations in index order): A's state
    i = iup + idw*DimUp is |map_up[iup]>|map_dw[idw]>; flipped it has the Fock number map_dw[idw] + 2**ns * map_up[iup]."""
    mu = np.asarray(map_up, dtype=np.int64)
    md = np.asarray(map_dw, dtype=np.int64)
    iup, idw = np.meshgrid(np.arange(mu.size), np.arange(md.size), indexing="xy")   # [idw, iup]: raveled, i = iup + idw*DimUp
    flipped = (md[idw] + (mu[iup] << ns)).ravel()
    return np.argsort(flipped, kind="stable")


def twin_vector(v, map_up, map_dw, ns):
    """v_B from v_A."""
    return np.asarray(v)[twin_order(map_up, map_dw, ns)]


def twin_matrix(map_up, map_dw, ns):
    """T with v_B = T v_A (a permutation matrix)."""
    order = twin_order(map_up, map_dw, ns)
    t = np.zeros((order.size, order.size))
    t[np.arange(order.size), order] = 1.0
    return t
