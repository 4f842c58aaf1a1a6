"""Cross-batch queue of negative keys for the global / circle losses (--neg_queue).

An (L, C) fp32 ring buffer on the device of key rows from earlier steps -- the step's mapped ``x_global`` rows, one per clip,
detached -- plus its state ``{head, valid}`` as two device int32, so that a captured step replays while the queue fills
(csrc/loss.hip: facl_contrast_pair_queue reads ``valid`` on the device, facl_queue_push advances the state there).  The buffer
is zero-initialised and holds finite values only: columns at or beyond ``valid`` have d/dsim exactly 0, and 0 * NaN in the
backward GEMM would poison the gradient."""
import torch

from . import _lib


class NegativeQueue:
    """``L`` slots of ``C`` floats, ``P`` rows per push (L % P == 0: a push never wraps inside itself)."""

    def __init__(self, L, C, P, device):
        L, C, P = int(L), int(C), int(P)
        if L < 1 or P < 1 or L % P:
            raise ValueError("the queue length must be a positive multiple of the rows per push (got L=%d, P=%d)" % (L, P))
        if C < 4 or C % 4:
            raise ValueError("the queue holds rows of a multiple of 4 floats (got C=%d)" % C)
        self.L, self.C, self.P = L, C, P
        self.buf = torch.zeros((L, C), dtype=torch.float32, device=device)       # never _lib.empty: see the module docstring
        self.state = torch.zeros(2, dtype=torch.int32, device=device)            # {head, valid}
        self._staged = None

    def stage(self, rows):
        """Remember the step's key rows (P, C); ``push()`` stores them once the backward has read the queue."""
        self._staged = rows

    def push(self, rows=None):
        """Copy ``rows`` (default: the staged ones) into the slots [head, head + P) and advance the state, on the device."""
        if rows is None:
            rows, self._staged = self._staged, None
            if rows is None:
                raise RuntimeError("NegativeQueue.push() without rows: nothing was staged")
        _lib.require_cuda(rows, self.buf)
        if rows.dtype != torch.float32 or tuple(rows.shape) != (self.P, self.C):
            raise ValueError("push takes a float32 (%d, %d) matrix, got %s %s" % (self.P, self.C, rows.dtype, tuple(rows.shape)))
        rows = rows.detach().contiguous()
        lib = _lib.load_library()
        _lib.check(lib.facl_queue_push(_lib.ptr(rows), self.P, self.C, _lib.ptr(self.buf), self.L, _lib.ptr(self.state),
                                       _lib.stream()), "facl_queue_push(P=%d, C=%d, L=%d)" % (self.P, self.C, self.L))

    def head_valid(self):
        """(head, valid) read back to the host (synchronises; tests and logs only)."""
        h, v = self.state.tolist()
        return int(h), int(v)

    def valid_rows(self):
        """The filled rows as a copy (synchronises): the argument ``queue=`` of the closed forms in utils_my."""
        return self.buf[:min(max(self.head_valid()[1], 0), self.L)].clone()

    def snapshot(self):
        return self.buf.clone(), self.state.clone()

    def restore(self, snap=None):
        """In place (a captured graph holds the addresses); ``None``: the empty queue."""
        if snap is None:
            self.buf.zero_()
            self.state.zero_()
        else:
            self.buf.copy_(snap[0])
            self.state.copy_(snap[1])
        self._staged = None
