"""Cross-batch queue of negative keys for the global / circle losses (--neg_queue).

An (L, C) fp32 ring buffer on the device of key rows from earlier steps -- the step's mapped ``x_global`` rows, one per clip,
detached -- plus its state ``{head, valid}`` as two device int32, so that a captured step replays while the queue fills
(csrc/loss.hip: facl_contrast_pair_queue reads ``valid`` on the device, facl_queue_push advances the state there).  The buffer
is zero-initialised and holds finite values only: columns at or beyond ``valid`` have d/dsim exactly 0, and 0 * NaN in the
backward GEMM would poison the gradient.

``with_ids``: the queue also owns ``ids``, an (L,) int32 tensor with the class id of the clip that pushed each row (-1: unknown,
and every slot before its first push), for the class-aware mask of the losses (facl_contrast_pair_queue_cls reads it,
facl_queue_push_ids writes it in front of every push)."""
import torch

from . import _lib


class NegativeQueue:
    """``L`` slots of ``C`` floats, ``P`` rows per push (L % P == 0: a push never wraps inside itself)."""

    def __init__(self, L, C, P, device, with_ids=False):
        L, C, P = int(L), int(C), int(P)
        if L < 1 or P < 1 or L % P:
            raise ValueError("the queue length must be a positive multiple of the rows per push (got L=%d, P=%d)" % (L, P))
        if C < 4 or C % 4:
            raise ValueError("the queue holds rows of a multiple of 4 floats (got C=%d)" % C)
        self.L, self.C, self.P = L, C, P
        self.buf = torch.zeros((L, C), dtype=torch.float32, device=device)       # never _lib.empty: see the module docstring
        self.state = torch.zeros(2, dtype=torch.int32, device=device)            # {head, valid}
        self.ids = torch.full((L,), -1, dtype=torch.int32, device=device) if with_ids else None
        self._staged = self._staged_ids = None

    def stage(self, rows, ids=None):
        """Remember the step's key rows (P, C) -- with ids: and their class ids (P,) int32; ``push()`` stores them once the
        backward has read the queue."""
        self._staged, self._staged_ids = rows, ids

    def push(self, rows=None, ids=None):
        """Copy ``rows`` (default: the staged ones) into the slots [head, head + P) and advance the state, on the device.  A
        queue with ids takes ``ids`` (P,) int32 with the rows and writes them into the same slots first (the same head)."""
        if rows is None:
            rows, ids = self._staged, self._staged_ids
            self._staged = self._staged_ids = None
            if rows is None:
                raise RuntimeError("NegativeQueue.push() without rows: nothing was staged")
        _lib.require_cuda(rows, self.buf)
        if rows.dtype != torch.float32 or tuple(rows.shape) != (self.P, self.C):
            raise ValueError("push takes a float32 (%d, %d) matrix, got %s %s" % (self.P, self.C, rows.dtype, tuple(rows.shape)))
        if (ids is not None) != (self.ids is not None):
            raise ValueError("a queue %s ids was pushed rows %s them" % (("without", "with") if self.ids is None else ("with", "without")))
        rows = rows.detach().contiguous()
        if ids is not None:
            _lib.require_cuda(ids)
            if ids.dtype != torch.int32 or tuple(ids.shape) != (self.P,) or not ids.is_contiguous():
                raise ValueError("push takes contiguous int32 (%d,) ids, got %s %s" % (self.P, ids.dtype, tuple(ids.shape)))
            _lib.call("facl_queue_push_ids", ids, self.P, self.ids, self.L, self.state, detail="P=%d, L=%d" % (self.P, self.L))
        _lib.call("facl_queue_push", rows, self.P, self.C, self.buf, self.L, self.state,
                  detail="P=%d, C=%d, L=%d" % (self.P, self.C, self.L))

    def head_valid(self):
        """(head, valid) read back to the host (synchronises; tests and logs only)."""
        h, v = self.state.tolist()
        return int(h), int(v)

    def valid_rows(self):
        """The filled rows as a copy (synchronises): the argument ``queue=`` of the closed forms in utils_my."""
        return self.buf[:min(max(self.head_valid()[1], 0), self.L)].clone()

    def valid_ids(self):
        """The ids of the filled rows as a copy (synchronises): the argument ``queue_classes=`` of the closed forms."""
        return self.ids[:min(max(self.head_valid()[1], 0), self.L)].clone()

    def snapshot(self):
        """(buf, state) -- with ids: (buf, state, ids) -- as copies."""
        snap = (self.buf.clone(), self.state.clone())
        return snap if self.ids is None else snap + (self.ids.clone(),)

    def restore(self, snap=None):
        """In place (a captured graph holds the addresses); ``None``: the empty queue.  A queue with ids takes the 3-tuple of
        its ``snapshot()``, one without the 2-tuple."""
        if snap is not None and len(snap) != (2 if self.ids is None else 3):
            raise ValueError("a queue %s ids restores a snapshot of %d entries, got %d"
                             % ("without" if self.ids is None else "with", 2 if self.ids is None else 3, len(snap)))
        if snap is None:
            self.buf.zero_()
            self.state.zero_()
            if self.ids is not None:
                self.ids.fill_(-1)
        else:
            self.buf.copy_(snap[0])
            self.state.copy_(snap[1])
            if self.ids is not None:
                self.ids.copy_(snap[2])
        self._staged = self._staged_ids = None
