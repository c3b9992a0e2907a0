"""The device-resident sampler (csrc/search.hip) at the C-ABI boundary, without a GPU: the entry points are exported and bound, reject bad
arguments before any launch (null device pointers never reach a kernel) and name themselves in the error text; the model's switch exists
and is off."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mr-blip_amd", "csrc", "libmrblip_hip.so")
NEW = ("mrblip_sample_topk", "mrblip_sample_topk_workspace_bytes", "mrblip_sample_advance")


def test_library_exports_the_sampler_entry_points():
    from mrblip import ops
    lib = ctypes.CDLL(LIB)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in ops.EXPORTS, n
    for fn in ("sample_topk", "sample_topk_workspace_bytes", "sample_advance"):
        assert callable(getattr(ops, fn)), fn
    lib.mrblip_abi_version.restype = ctypes.c_int
    assert lib.mrblip_abi_version() == 1


def test_header_and_bindings_still_agree():
    import test_abi_cpu
    test_abi_cpu.test_library_exports_every_declared_symbol()
    test_abi_cpu.test_python_bindings_cover_the_header()
    assert set(NEW) <= set(test_abi_cpu._declared())


def _topk(R, top_k, V, ws_bytes=0, ws=None):
    from mrblip import ops
    # logits, ldl, seqs, lds, R, V, cur_len, top_k, min_length, eos_id, penalty, cand_score, cand_index, ws, ws_bytes, stream
    return ops._sample_topk(None, V, None, 8, R, V, 1, top_k, 1, 1, 1.0, None, None, ws, ws_bytes, None)


def _advance(R, top_k, V, temperature=1.0, top_p=0.9, lds=8, cur_len=1):
    from mrblip import ops
    # cand_score, cand_index, seq, lds, tokens, unfinished, length, done_count, uniforms, seed, R, V, top_k, cur_len, eos, pad, T, top_p, greedy
    return ops._sample_advance(None, None, None, lds, None, None, None, None, None, 0, R, V, top_k, cur_len, 1, 0, temperature, top_p, 0, None)


BAD_SHAPES = [(3, 0, 100, b"top_k = 0"), (3, 65, 100, b"top_k = 65"), (3, 50, 131073, b"V = 131073"), (257, 50, 100, b"R = 257")]


@pytest.mark.parametrize("R,top_k,V,what", BAD_SHAPES)
def test_sampler_entry_points_reject_bad_shapes_before_any_launch(R, top_k, V, what):
    from mrblip import ops
    lib = ops._lib
    assert _topk(R, top_k, V) == -1
    assert b"mrblip_sample_topk" in lib.mrblip_last_error() and what in lib.mrblip_last_error(), lib.mrblip_last_error()
    assert _advance(R, top_k, V) == -1
    assert b"mrblip_sample_advance" in lib.mrblip_last_error() and what in lib.mrblip_last_error(), lib.mrblip_last_error()
    assert lib.mrblip_sample_topk_workspace_bytes(R, top_k, V) == -1
    with pytest.raises(ops.MrblipError):
        ops.sample_topk_workspace_bytes(R, top_k, V)


def test_sample_advance_rejects_a_temperature_that_is_not_positive():
    from mrblip import ops
    lib = ops._lib
    for T in (0.0, -0.5):
        assert _advance(3, 50, 100, temperature=T) == -1
        assert b"mrblip_sample_advance: temperature" in lib.mrblip_last_error(), lib.mrblip_last_error()
    assert _advance(3, 50, 100, top_p=0.0) == -1 and b"top_p" in lib.mrblip_last_error()
    # a sequence row without room for the new token, and the built-in draws past their 256 steps
    assert _advance(3, 50, 100, lds=4, cur_len=4) == -1 and b"hold no position 4" in lib.mrblip_last_error()
    assert _advance(3, 50, 100, lds=400, cur_len=257) == -1 and b"256 steps" in lib.mrblip_last_error()
    # good arguments with null buffers are still an argument error, not a launch
    assert _advance(3, 50, 100) == -1 and b"mrblip_sample_advance: null buffer" in lib.mrblip_last_error()


def test_sample_topk_rejects_a_workspace_that_is_too_small():
    from mrblip import ops
    lib = ops._lib
    need = ops.sample_topk_workspace_bytes(3, 50, 32128)
    assert need == 8 * 3 * 16 * 50
    assert ops.sample_topk_workspace_bytes(3, 50, 40) == 8 * 3 * 1 * 40          # k = min(top_k, V)
    assert ops.sample_topk_workspace_bytes(3, 50, 2049) == 8 * 3 * 2 * 50
    # (every pointer non-null but never dereferenced: the size check comes before any launch)
    fake = ctypes.c_void_p(4096)
    rc = ops._sample_topk(fake, 32128, fake, 8, 3, 32128, 1, 50, 1, 1, 1.0, fake, fake, fake, need - 1, None)
    assert rc == -1 and b"mrblip_sample_topk" in lib.mrblip_last_error() and str(need).encode() in lib.mrblip_last_error(), lib.mrblip_last_error()
    assert _topk(3, 50, 32128) == -1 and b"mrblip_sample_topk: null buffer" in lib.mrblip_last_error()


def test_generate_device_sample_switch_exists_and_is_off():
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    cls = registry.get_model_class("blip2_mr")
    assert cls.generate_device_sample is False
    assert cls.generate_device_search is False
    from mrblip.search import DeviceSampleSearch
    for name in ("tokens", "step", "done_count_async", "finished", "steps_after_done", "finalize", "reset"):
        assert hasattr(DeviceSampleSearch, name), name
