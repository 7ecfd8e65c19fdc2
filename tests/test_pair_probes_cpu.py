"""Paired probe runs without a GPU (include/hxv.h: hxv_lanczos_tridiag_pair_probes): the symbol is exported and listed, and a NULL handle is
refused before the device is touched."""
import ctypes


def test_new_symbol_is_exported_and_listed(built):
    import hxv

    lib = ctypes.CDLL(str(hxv.LIB_PATH))
    assert "hxv_lanczos_tridiag_pair_probes" in hxv.EXPORTS and hasattr(lib, "hxv_lanczos_tridiag_pair_probes")
    assert hasattr(hxv.HxvSector, "lanczos_tridiag_pair_probes")


def test_null_handle_is_refused(built):
    import hxv

    L = hxv.load_library()
    assert L.hxv_lanczos_tridiag_pair_probes(None, None, None, 0, None, 1, None, None, None, None, None, None, 1e-12, None, None) == 1   # HXV_ERR_ARG
    assert b"hxv_lanczos_tridiag_pair_probes" in L.hxv_last_error()
