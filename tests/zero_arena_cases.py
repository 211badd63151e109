"""A zero arena with guard bands, for tests/test_zero_arena_gpu.py (a plain helper module).

``GuardedArena`` serves every request ``GUARD`` floats longer than asked and hands out the front part: a kernel that writes
past its extent then lands in memory the arena owns (a guard band, alignment padding or the tail) instead of in a
neighbour's gradient, and ``dirty_guard_elements`` reads it back.  Nothing here provokes a fault: an overrun of up to
``GUARD`` floats stays inside the one allocation."""
import contextlib

import torch

from salience_detr_amd import zero_arena as Z

GUARD = 64   # floats behind every slice (the arena's own alignment leaves 0 .. 63)


class GuardedArena(Z.ZeroArena):
    def __init__(self, device, slack: float = 0.0):
        super().__init__(device, slack)
        self.extents = []     # (offset, numel) of every slice served in the current step
        self.takes = 0        # take() calls of the current step

    @contextlib.contextmanager
    def step(self):
        self.extents, self.takes = [], 0
        with super().step():
            yield self

    def take(self, numel):
        # (the sizing pass and the served passes both come through here: demand and offsets stay consistent)
        self.takes += 1
        off = self.off
        t = super().take(numel + GUARD)
        if t is None:
            return None
        self.extents.append((off, numel))
        return t[:numel]


def dirty_guard_elements(arena) -> int:
    """Non-zero or NaN elements of ``arena.buf`` outside the slices served in its last step: every guard band, all
    alignment padding and the tail."""
    outside = torch.ones(arena.buf.numel(), dtype=torch.bool, device=arena.buf.device)
    for off, numel in arena.extents:
        outside[off:off + numel] = False
    return int((arena.buf[outside] != 0).sum().item())     # (NaN != 0 holds)


def assert_fully_served(arena) -> None:
    """The arena's last step got every fp32 request from the buffer."""
    assert arena.takes > 0 and len(arena.extents) == arena.takes == arena.fills_saved, \
        (arena.takes, len(arena.extents), arena.fills_saved)
    assert arena.demand <= arena.buf.numel(), (arena.demand, arena.buf.numel())
    ends = [off + numel + GUARD for off, numel in arena.extents]
    assert all(e <= nxt for e, (nxt, _) in zip(ends, arena.extents[1:])) and ends[-1] <= arena.buf.numel()


def run_served(fn, device):
    """``fn()`` under ``arena.step()`` twice -- once to size a fresh ``GuardedArena``, once served from it; returns the
    second pass's result and the arena."""
    arena = GuardedArena(device)
    with arena.step():
        fn()
    assert arena.fills_saved == 0 and arena.takes > 0, "the sizing pass asked the arena for nothing"
    with arena.step():
        out = fn()
    assert_fully_served(arena)
    return out, arena
