"""The device-resident beam search (csrc/search.hip) at the C-ABI boundary, without a GPU: the four entry points are exported, reject
bad shapes before any launch (null device pointers never reach a kernel) and name themselves in the error text; the model's switch
exists and is off."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mr-blip_amd", "csrc", "libmrblip_hip.so")
NEW = ("mrblip_beam_topk", "mrblip_beam_advance", "mrblip_beam_finalize", "mrblip_kv_gather_rows")


def test_library_exports_the_search_entry_points():
    from mrblip import ops
    lib = ctypes.CDLL(LIB)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in ops.EXPORTS, n
    for fn in ("beam_topk", "beam_advance", "beam_finalize", "kv_gather_rows"):
        assert callable(getattr(ops, fn)), fn


def test_beam_topk_rejects_bad_shapes_before_any_launch():
    from mrblip import ops
    lib = ops._lib

    def topk(R, K, V):
        return ops._beam_topk(None, V, None, None, 8, R, K, V, 1, 1, 1, 1.0, None, None, None, 0, None)

    for R, K, V, what in ((5, 5, 9, "V < 2K"), (4, 0, 48, "K = 0"), (17, 17, 48, "K = 17"), (7, 5, 48, "R % K != 0")):
        assert topk(R, K, V) == -1, what
        assert b"mrblip_beam_topk" in lib.mrblip_last_error(), (what, lib.mrblip_last_error())
    # a good shape with null buffers is still an argument error, not a launch
    assert topk(5, 5, 48) == -1 and b"mrblip_beam_topk" in lib.mrblip_last_error()


def test_the_other_search_entry_points_check_their_arguments():
    from mrblip import ops
    lib = ops._lib
    n14 = (None,) * 14
    assert ops._beam_advance(*n14[:4], 8, *n14[:9], 1, 17, 48, 1, 1, 0, 1.0, None) == -1 and b"mrblip_beam_advance" in lib.mrblip_last_error()
    assert ops._beam_advance(*n14[:4], 4, *n14[:9], 1, 2, 48, 4, 1, 0, 1.0, None) == -1 and b"mrblip_beam_advance" in lib.mrblip_last_error()
    assert ops._beam_finalize(None, 8, None, None, None, None, None, None, 1, 2, 3, 1.0, 3, None, None) == -1
    assert b"mrblip_beam_finalize" in lib.mrblip_last_error()
    assert ops._kv_gather_rows(None, None, None, 4, 5, 32, 12, 1, None) == -1 and b"mrblip_kv_gather_rows" in lib.mrblip_last_error()
    assert ops._kv_gather_rows(None, None, None, 4, 5, 32, 16, 33, None) == -1 and b"mrblip_kv_gather_rows" in lib.mrblip_last_error()
    assert ops.beam_topk_workspace_bytes(5, 5, 32128) == 4 * 5 * 16 * 22


def test_generate_device_search_switch_exists_and_is_off():
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    cls = registry.get_model_class("blip2_mr")
    assert cls.generate_device_search is False
    assert cls.generate_cross_cache is True and cls.generate_self_cache is True
