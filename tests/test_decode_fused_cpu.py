"""The fused cached self-attention of generate's decode step (csrc/decode.hip) without a GPU: the export, the host-side argument
validation of the C ABI (nothing below reaches a launch: every call is rejected before it) and the model's two switches."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mr-blip_amd", "csrc", "libmrblip_hip.so")
NAME = "mrblip_decode_self_attention"

# fake, 16-byte aligned, distinct addresses: validation only compares them and looks at their alignment
KV_A, KV_B, QKV, OUT, LUT, PAR, POS = (0x10000 * (i + 1) for i in range(7))


def _call(kv_src=KV_A, kv_dst=KV_A, qkv=QKV, out=OUT, lut=LUT, parents=None, pos_dev=None, pos=3, layers=2, layer=1, R=3, Lmax=32, H=2, D=16,
          ldq=None, ldo=None):
    from mrblip import ops
    inner = H * D
    return ops._decode_self_attn(kv_src, kv_dst, qkv, 3 * inner if ldq is None else ldq, out, inner if ldo is None else ldo, lut, parents, pos_dev,
                                 pos, layers, layer, R, Lmax, H, D, 1.0, None)


def test_export_is_in_the_header_the_library_and_the_bindings():
    from mrblip import ops, torch_ops
    assert hasattr(ctypes.CDLL(LIB), NAME)
    assert NAME in ops.EXPORTS and callable(ops.decode_self_attention)
    header = open(os.path.join(ROOT, "include", "mrblip_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert "decode_self_attention" in torch_ops.OPS
    import torch
    s = str(torch.ops.mrblip.decode_self_attention.default._schema)
    assert s.count("!") == 2, s      # kv_dst and out are declared as mutated


def test_bad_arguments_are_rejected_before_any_launch():
    from mrblip import ops
    lib = ops._lib
    cases = {
        "null cache": dict(kv_src=None, kv_dst=None),
        "null qkv": dict(qkv=None),
        "null out": dict(out=None),
        "null lut": dict(lut=None),
        "D = 12": dict(D=12),
        "D = 136": dict(D=136),
        "pos = Lmax": dict(pos=32),
        "pos = -1": dict(pos=-1),
        "layer = layers": dict(layer=2),
        "kv_src == kv_dst with parents": dict(parents=PAR),
        "kv_src != kv_dst without parents": dict(kv_dst=KV_B),
        "ldq < 3 * inner": dict(ldq=3 * 32 - 8),
        "ldo < inner": dict(ldo=24),
        "unaligned out": dict(out=OUT + 2),
    }
    for what, kw in cases.items():
        assert _call(D=12) == -1 and b"D = 12" in lib.mrblip_last_error()      # (so that the text asserted next is this case's own)
        assert _call(**kw) == -1, what
        err = lib.mrblip_last_error()
        assert NAME.encode() in err and (what.startswith("D = ") or b"D = 12" not in err), (what, err)
    # the host position is not looked at when the device word is given — the call then fails on something else
    assert _call(pos=32, pos_dev=POS, D=12) == -1 and b"D = 12" in lib.mrblip_last_error()


def test_both_switches_default_to_false_and_are_read_from_the_model_config():
    import inspect
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    cls = registry.get_model_class("blip2_mr")
    assert cls.generate_fused_decode is False and cls.generate_graph_decode is False
    src = inspect.getsource(cls.from_config)
    for key in ("generate_fused_decode", "generate_graph_decode"):
        assert re.search(r"model\.%s\s*=\s*bool\(cfg\.get\(\"%s\",\s*False\)\)" % (key, key), src), key
