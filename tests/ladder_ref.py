"""Host restatement of the Green's-function start vectors (ED_GF_NORMAL.f90:180-199): the reference the device ladder operators
are checked against, bit for bit (tests/test_gpu_lanczos.py, tests/test_gpu_layout_contract.py)."""
import numpy as np


def apply_op(psi, maps_from, maps_to, pos, spin, create):
    """c / c^dagger on orbital `pos` (0-based) of one spin: vvinit(j) = sgn*psi(i), ED_GF_NORMAL.f90:180-199.
    maps_* = (map_up, map_dw) of the two sectors.  Sign counts occupied orbitals below pos on the same spin only."""
    mu_f, md_f = maps_from
    mu_t, md_t = maps_to
    du_f, dd_f, du_t, dd_t = len(mu_f), len(md_f), len(mu_t), len(md_t)
    P = psi.reshape((du_f, dd_f), order="F")
    out = np.zeros((du_t, dd_t), dtype=complex)
    src = mu_f if spin == 0 else md_f
    dst = mu_t if spin == 0 else md_t
    pos_of = {int(s): k for k, s in enumerate(dst)}
    bit = 1 << pos
    for k, s in enumerate(src):
        s = int(s)
        occ = bool(s & bit)
        if occ == create:
            continue
        sgn = -1.0 if bin(s & (bit - 1)).count("1") % 2 else 1.0
        t = pos_of[(s | bit) if create else (s & ~bit)]
        if spin == 0:
            out[t, :] += sgn * P[k, :]
        else:
            out[:, t] += sgn * P[:, k]
    return out.reshape(-1, order="F")
