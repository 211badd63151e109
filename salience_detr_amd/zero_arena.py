"""One zero fill per training step (round 6, VERDICT r5 item 7: "one multi-tensor zero").

The autograd nodes of the training step (``util/engine.py:44-64`` in the reference: forward, loss, backward, optimizer)
need ~150 zero-initialised fp32 buffers per step here: the split-reduction outputs of the fp32-accurate GEMMs (their
slices add with atomics), every weight / bias gradient (the same, ``linear_x3.py``), LayerNorm's ``dw | db`` pair
(``layer_norm_train.py``) and the deformable attention's ``grad_value`` (``ms_deform_im2col_cuda.cuh:290-392`` accumulates
into it).  As ``torch.zeros`` calls they were ~150 fill launches of 4.5 us each inside the replayed hipGraph (0.68 ms of a
15.4 ms step).  A ``ZeroArena`` serves them as slices of ONE buffer that is cleared by ONE fill kernel when the step
begins.

Protocol: ``with arena.step(): forward; backward`` -- the first step only measures the demand (its requests fall
through to ``torch.zeros``), the buffer is allocated when that step ends, every later step clears it and hands out
slices in request order.  The requests of a step must not outlive the NEXT ``step()`` entry: gradients that become
``p.grad`` are consumed by the optimizer (or packed into the flat all-reduce buffer) before the next step begins, and the
step must start with ``p.grad = None`` (``optimizer.zero_grad(set_to_none=True)``, the framework's default) -- a
``p.grad`` kept across steps would alias the slice the next backward writes.  Without an active arena ``zeros()`` is
``torch.zeros``.

Capture: inside a captured hipGraph the fill is one captured kernel and the slices are static addresses, which is what
replay needs -- so the order is sizing step(s) first, eager, THEN the capture.  ``step()`` notes whether it was entered
while the current stream is capturing, and two things that would silently break a replay raise instead.  (1) While
capturing, a request the buffer cannot serve (no sizing step yet, or more than the sizing step asked for) raises: falling
through to ``torch.zeros`` would put a fresh block's memset node into the graph, which replay does not reproduce
(``graph_guard.py``).  (2) Once a step of this arena has been captured, the buffer is never reallocated: an eager step
whose demand exceeds it raises when it ends (the graph holds the old buffer's addresses) -- create a new arena, size it
with the larger step, and capture again.
"""
import contextlib
from typing import Optional

import torch

_active: Optional["ZeroArena"] = None
_ALIGN = 64   # elements: 256-byte slices (the GEMM's 16-byte operand rule with room to spare)


class ZeroArena:
    def __init__(self, device, slack: float = 0.0):
        self.device = torch.device(device)
        self.buf: Optional[torch.Tensor] = None
        self.off = 0          # elements handed out in the current step
        self.demand = 0       # elements requested in the current step (served or not)
        self.slack = slack
        self.fills_saved = 0  # requests served from the buffer in the last step
        self.captured = False   # a step of this arena lives in a hipGraph: ``buf`` must stay where it is
        self._capturing = False  # the current step was entered while the stream is capturing

    @contextlib.contextmanager
    def step(self):
        global _active
        if _active is not None:
            raise RuntimeError("ZeroArena.step: another arena's step is active")
        self.off = self.demand = self.fills_saved = 0
        self._capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if self.buf is not None:
            self.buf.zero_()          # the step's ONE fill kernel
        _active = self
        try:
            yield self
        finally:
            _active = None
            capturing, self._capturing = self._capturing, False
        # (reached only when the body raised nothing)
        have = 0 if self.buf is None else self.buf.numel()
        if (self.buf is None or self.demand > have) and not capturing:   # (a capturing step that got here asked for nothing new)
            if self.captured:
                raise RuntimeError(
                    "ZeroArena.step: demand grew after capture (%d elements asked for, the buffer holds %d): a captured "
                    "graph holds this buffer's addresses, so it is not reallocated -- re-create the arena, size it with "
                    "this step and re-capture" % (self.demand, have))
            # measured demand of this step: allocate (or grow) for the next one
            n = int(self.demand * (1.0 + self.slack)) + _ALIGN
            self.buf = torch.empty(n, dtype=torch.float32, device=self.device)
        self.captured = self.captured or capturing

    def take(self, numel: int) -> Optional[torch.Tensor]:
        n = (numel + _ALIGN - 1) // _ALIGN * _ALIGN
        self.demand += n
        if self.buf is None or self.off + n > self.buf.numel():
            if self._capturing:
                raise RuntimeError(
                    "ZeroArena: a request of %d elements cannot be served while the stream is capturing (%s): run one "
                    "sizing step before capturing -- torch.zeros of a fresh block is a memset node, which a replayed "
                    "graph does not reproduce" % (numel, "no sizing step yet" if self.buf is None else
                                                  "%d of %d elements handed out" % (self.off, self.buf.numel())))
            return None
        out = self.buf[self.off:self.off + numel]
        self.off += n
        self.fills_saved += 1
        return out


def _same_device(d: torch.device, e: torch.device) -> bool:
    if d.type != e.type:
        return False
    if d.type != "cuda":
        return True
    cur = torch.cuda.current_device()
    return (cur if d.index is None else d.index) == (cur if e.index is None else e.index)


def zeros(shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """``torch.zeros(shape, dtype=dtype, device=device)``; inside ``ZeroArena.step()`` on the arena's device and for fp32
    a slice of the step's pre-cleared buffer."""
    if isinstance(shape, int):
        shape = (shape,)
    a = _active
    if a is not None and dtype == torch.float32 and device is not None and _same_device(torch.device(device), a.device):
        numel = 1
        for d in shape:
            numel *= int(d)
        if numel > 0:
            t = a.take(numel)
            if t is not None:
                return t.view(tuple(int(d) for d in shape))
    return torch.zeros(shape, dtype=dtype, device=device)


def zeros_like(t: torch.Tensor) -> torch.Tensor:
    return zeros(tuple(t.shape), t.dtype, t.device)
