"""The gradient guard (csrc/optim.hip, mrblip/grad_guard.py) without a GPU: the three exports, the host-side argument validation of the C
ABI (nothing below reaches a launch: every call is rejected before it), the torch.ops registration, and the switches of FlatAdamW and of
the run config."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mrblip_grad_stats_workspace_bytes", "mrblip_grad_sumsq", "mrblip_optim_prepare")
# fake, 16-byte aligned, distinct "device pointers": validation only looks at null-ness and alignment
G, WS, HIN, STATE, HOUT, GUARD = (0x10000 * (i + 1) for i in range(6))


def test_exports_are_in_the_header_the_library_and_the_bindings():
    from mrblip import ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrblip_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(ops.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b(int|long long)\s+%s\s*\(" % n, hdr), n
        assert n in ops.EXPORTS, n
        assert hasattr(lib, n), n
    assert callable(ops.grad_sumsq) and callable(ops.optim_prepare) and callable(ops.grad_norm)
    # the documented layout: 16 bytes per 16384-element chunk, at least one record
    C = ops.GRAD_CHUNK
    assert C == 16384 and ops.OPTIM_STATE_WORDS == 8
    for n, chunks in ((0, 1), (1, 1), (C - 1, 1), (C, 1), (C + 1, 2), (3 * C + 5, 4), (2 ** 20 + 17, 65), (1 << 33, 1 << 19)):
        assert ops.grad_stats_workspace_bytes(n) == 16 * chunks, n
    with pytest.raises(ops.MrblipError):
        ops.grad_stats_workspace_bytes(-1)


def _sumsq(g=G, n=100, ws=WS, ws_bytes=16):
    from mrblip import ops
    return ops._grad_sumsq(g, n, ws, ws_bytes, None)


def _prepare(ws=WS, n=100, hin=HIN, b1=0.9, b2=0.999, max_norm=0.0, guard=None, state=STATE, hout=HOUT):
    from mrblip import ops
    return ops._optim_prepare(ws, n, hin, b1, b2, max_norm, guard, state, hout, None)


def test_bad_arguments_are_rejected_before_any_launch():
    from mrblip import ops
    err = ops._lib.mrblip_last_error
    for what, kw, msg in (("null g", dict(g=None), b"null operand"), ("null workspace", dict(ws=None), b"null operand"),
                          ("n < 0", dict(n=-1), b"n = -1"), ("workspace too small", dict(n=16385, ws_bytes=16), b"32 needed"),
                          ("no workspace bytes", dict(ws_bytes=0), b"16 needed"), ("g off a float boundary", dict(g=G + 2), b"unaligned"),
                          ("workspace off 16 bytes", dict(ws=WS + 8), b"unaligned")):
        assert _sumsq(**kw) == -1, what
        assert b"mrblip_grad_sumsq" in err() and msg in err(), (what, err())
    for what, kw, msg in (("null workspace", dict(ws=None), b"null operand"), ("null hyper_in", dict(hin=None), b"null operand"),
                          ("null state", dict(state=None), b"null operand"), ("null hyper_out", dict(hout=None), b"null operand"),
                          ("n < 0", dict(n=-5), b"n = -5"), ("beta1 = 1", dict(b1=1.0), b"outside [0, 1)"),
                          ("beta1 < 0", dict(b1=-0.1), b"outside [0, 1)"), ("beta2 = 1.5", dict(b2=1.5), b"outside [0, 1)"),
                          ("beta2 NaN", dict(b2=float("nan")), b"outside [0, 1)"), ("max_norm NaN", dict(max_norm=float("nan")), b"max_norm is NaN"),
                          ("state off a word", dict(state=STATE + 1), b"unaligned"), ("guard off a word", dict(guard=GUARD + 2), b"unaligned")):
        assert _prepare(**kw) == -1, what
        assert b"mrblip_optim_prepare" in err() and msg in err(), (what, err())


def test_python_wrappers_check_their_tensors_before_the_device():
    from mrblip import ops

    with pytest.raises(ops.MrblipError, match="cuda"):      # CPU tensors: refused, there is no CPU fallback
        ops.grad_sumsq(torch.zeros(8), torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ops.MrblipError, match="cuda"):
        ops.grad_norm(torch.zeros(8))
    with pytest.raises(ops.MrblipError, match="cuda"):
        ops.optim_prepare(torch.zeros(16, dtype=torch.uint8), 8, torch.zeros(2), torch.zeros(8, dtype=torch.int32), torch.zeros(4))


def test_torch_op_schema_fake_shape_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mrblip import torch_ops

    assert "grad_norm" in torch_ops.OPS
    sch = torch.ops.mrblip.grad_norm.default._schema
    assert sch.name == "mrblip::grad_norm" and "!" not in str(sch), str(sch)            # nothing mutated
    assert [a.name for a in sch.arguments] == ["g"] and len(sch.returns) == 2, str(sch)
    with FakeTensorMode():
        norm, bad = torch.ops.mrblip.grad_norm(torch.empty(1000))
        assert norm.shape == (1,) and norm.dtype == torch.float32 and bad.shape == (1,) and bad.dtype == torch.int32
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mrblip.grad_norm(torch.zeros(8))


def _stub_model():
    eng = types.SimpleNamespace(flat=torch.zeros(1000))
    return types.SimpleNamespace(engine=eng)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "abc", True])
def test_flat_adamw_and_the_run_keys_reject_a_bad_max_grad_norm(bad):
    import lavis  # noqa: F401
    from lavis.runners.runner_base import FlatAdamW, grad_guard_options

    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        grad_guard_options({"max_grad_norm": bad})
    with pytest.raises(ValueError, match="max_grad_norm"):
        grad_guard_options({"grad_guard": True, "max_grad_norm": bad})


def test_switches_default_to_off_and_max_grad_norm_alone_turns_the_guard_on():
    import inspect
    import lavis  # noqa: F401
    from lavis.runners.runner_base import FlatAdamW, RunnerBase, grad_guard_options
    from mrblip.engine import MrBlipEngine

    off = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05)
    assert off.grad_guard is False and off.guard is None and off.max_grad_norm is None and off.stats() is None
    assert set(off.state_dict()) == {"t", "m", "v", "lr"}                                 # the unguarded checkpoint is what it was
    on = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05, grad_guard=True)
    assert on.grad_guard is True and on.max_grad_norm is None and on.guard.max_consecutive_skips == 8 and on.stats() is None
    clip = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05, max_grad_norm=2)
    assert clip.grad_guard is True and clip.max_grad_norm == 2.0 and isinstance(clip.max_grad_norm, float)
    assert clip.guard.state.numel() == 8 and clip.guard.state.dtype == torch.int32 and clip.guard.ws.numel() == 16
    # the run keys
    assert grad_guard_options({}) == {"grad_guard": False, "max_grad_norm": None}
    assert grad_guard_options({"grad_guard": True}) == {"grad_guard": True, "max_grad_norm": None}
    assert grad_guard_options({"max_grad_norm": "0.5"}) == {"grad_guard": False, "max_grad_norm": 0.5}     # (FlatAdamW turns the guard on)
    assert grad_guard_options({"max_grad_norm": None}) == {"grad_guard": False, "max_grad_norm": None}
    assert "grad_guard_options(run)" in inspect.getsource(RunnerBase.__init__)
    # the engine's own step: both switches off by default
    sig = inspect.signature(MrBlipEngine.optimizer_step)
    assert sig.parameters["grad_guard"].default is False and sig.parameters["max_grad_norm"].default is None


def test_checkpoint_clock_round_trip_between_guarded_and_unguarded():
    import lavis  # noqa: F401
    from lavis.runners.runner_base import FlatAdamW

    plain = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05)
    plain.t = 7
    g = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05, grad_guard=True)
    g.load_state_dict(plain.state_dict())                                                 # written without the guard: applied = t
    assert g.guard.read()["applied_steps"] == 7 and g.guard.read()["skipped_steps"] == 0
    g.guard.set_clock(9, 3)
    sd = g.state_dict()
    assert sd["t"] == 9 and sd["skipped"] == 3 and set(sd) == {"t", "skipped", "m", "v", "lr"}
    plain.load_state_dict(sd)                                                             # ... and the other way round
    assert plain.t == 9
    g2 = FlatAdamW(_stub_model(), lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
    g2.load_state_dict(sd)
    st = g2.guard.read()
    assert st["applied_steps"] == 9 and st["skipped_steps"] == 3 and st["consecutive_skips"] == 0 and not math.isnan(st["grad_norm"])
