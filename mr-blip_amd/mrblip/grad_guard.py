"""The opt-in gradient guard of the optimizer step (csrc/optim.hip), shared by ``FlatAdamW`` (lavis/runners/runner_base.py)
and ``MrBlipEngine.optimizer_step``: one pass over the flat gradient gives the global norm and the count of non-finite values, one small
launch decides on the device whether the step is applied, counts it (the device counter is the optimizer clock), computes AdamW's bias
terms and the clip factor — and the unchanged guarded AdamW kernel does the rest.  The counterpart of what the reference's GradScaler does
besides scaling: it checks the gradients for inf / nan and skips the optimizer step (runner_base.py:127-132, moment_retrieval.py:221-233).

Nothing here waits for the device except ``read()`` (checkpoints, tests) and ``stats(block=True)``: each step's state block travels to
pinned host memory behind the step and is looked at when it has arrived."""
import math
from typing import Optional

import torch

from . import ops

STATE_FIELDS = ("skip", "applied", "skipped", "nonfinite", "norm", "clip", "consecutive_skips")   # words 0..6 of the state block


def check_max_grad_norm(max_grad_norm) -> Optional[float]:
    """None, or the value as a finite float above 0 (ValueError otherwise)"""
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool):
        raise ValueError(f"max_grad_norm must be a finite number above 0, got {max_grad_norm!r}")
    try:
        v = float(max_grad_norm)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be a finite number above 0, got {max_grad_norm!r}") from None
    if not math.isfinite(v) or v <= 0.0:
        raise ValueError(f"max_grad_norm must be a finite number above 0, got {max_grad_norm!r}")
    return v


def decode_state(words) -> dict:
    """the 8 int32 words of a state block (host tensor) -> the dict ``stats()`` returns"""
    w = words.view(torch.int32)
    f = words.view(torch.float32)
    u = lambda i: int(w[i]) & 0xFFFFFFFF   # noqa: E731
    return {"grad_norm": float(f[4]), "clip": float(f[5]), "nonfinite": u(3), "skipped_step": bool(u(0)), "applied_steps": u(1),
            "skipped_steps": u(2), "consecutive_skips": u(6)}


class GradGuard:
    """Device block + deferred host view of one optimizer's guard.  ``n``: elements of the flat gradient it will be run over."""

    RING = 4   # pinned slots for the state's way to the host: a slot is reused four steps later, long after its copy has landed

    def __init__(self, device, n: int, max_grad_norm=None, max_consecutive_skips: int = 8):
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.max_consecutive_skips = int(max_consecutive_skips)
        if self.max_consecutive_skips < 1:
            raise ValueError(f"max_consecutive_skips must be at least 1, got {max_consecutive_skips!r}")
        self.device, self.n = torch.device(device), int(n)
        self.state = torch.zeros(ops.OPTIM_STATE_WORDS, dtype=torch.int32, device=self.device)
        self.hyper_in = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.ws = torch.empty(ops.grad_stats_workspace_bytes(self.n), dtype=torch.uint8, device=self.device)
        self._slots = None          # [pinned int32 [8], event or None, sequence number]
        self._seq = 0
        self._newest = None         # (sequence number, dict) of the newest state that has arrived

    # ---- device side
    def skip_word(self) -> torch.Tensor:
        """the word the guarded AdamW takes as its guard (0 = apply)"""
        return self.state[0:1]

    def prepare(self, g: torch.Tensor, lr: float, grad_scale: float, betas, hyper_out: torch.Tensor, guard_in: Optional[torch.Tensor] = None):
        """uploads {lr, grad_scale} (non-blocking), runs the two launches over ``g`` and posts the state's copy to the host.  Afterwards
        ``hyper_out`` is AdamW's hyper block and ``skip_word()`` its guard."""
        assert g.numel() == self.n, (g.numel(), self.n)
        self.hyper_in.copy_(torch.tensor([lr, grad_scale], dtype=torch.float32).pin_memory(), non_blocking=True)
        ops.grad_sumsq(g, self.ws)
        ops.optim_prepare(self.ws, self.n, self.hyper_in, self.state, hyper_out, betas[0], betas[1], self.max_grad_norm or 0.0, guard=guard_in)
        self._post()

    def read(self) -> dict:
        """the device block, now (blocking: checkpoints and tests)"""
        return decode_state(self.state.cpu())

    def set_clock(self, applied: int, skipped: int = 0):
        """checkpoint -> device block"""
        self.state.copy_(torch.tensor([0, int(applied), int(skipped), 0, 0, 0, 0, 0], dtype=torch.int64).to(torch.int32))
        self._newest = None
        if self._slots is not None:
            for s in self._slots:
                s[1] = None

    # ---- host side: never waits unless asked to
    def _post(self):
        if self._slots is None:
            self._slots = [[torch.zeros(ops.OPTIM_STATE_WORDS, dtype=torch.int32).pin_memory(), None, 0] for _ in range(self.RING)]
        self._seq += 1
        slot = self._slots[self._seq % self.RING]
        if slot[1] is not None and not slot[1].query():
            return                                   # (its copy of four steps ago is still in flight: this step's state is not posted)
        self._collect(slot)
        slot[0].copy_(self.state, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        slot[2] = self._seq

    def _collect(self, slot):
        if slot[1] is not None:
            if self._newest is None or slot[2] > self._newest[0]:
                self._newest = (slot[2], decode_state(slot[0]))
            slot[1] = None

    def poll(self, block: bool = False):
        """takes in every state that has arrived (block: waits for the newest one posted) and raises RuntimeError when the newest shows
        max_consecutive_skips skipped steps in a row: a run that trains nothing must not look healthy"""
        if self._slots is not None:
            if block:
                pending = [s for s in self._slots if s[1] is not None]
                if pending:
                    max(pending, key=lambda s: s[2])[1].synchronize()
            for s in self._slots:
                if s[1] is not None and s[1].query():
                    self._collect(s)
        if self._newest is not None and self._newest[1]["consecutive_skips"] >= self.max_consecutive_skips:
            st = self._newest[1]
            raise RuntimeError(f"gradient guard: {st['consecutive_skips']} optimizer steps in a row were skipped (max_consecutive_skips = "
                               f"{self.max_consecutive_skips}); the last gradient norm was {st['grad_norm']} with {st['nonfinite']} non-finite "
                               f"value(s); {st['applied_steps']} steps applied, {st['skipped_steps']} skipped so far")

    def stats(self, block: bool = False) -> Optional[dict]:
        self.poll(block)
        if self._newest is None:
            return None
        st = dict(self._newest[1])
        st.pop("consecutive_skips")
        return st
