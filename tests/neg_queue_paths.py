"""Which path facl_contrast_pair_queue's launcher takes for a shape, from the launcher's own constants: they are read out of
csrc/loss.hip, so the tests that place their cases around a threshold follow it when it moves."""
import os
import re

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "facl_amd", "csrc", "loss.hip")


def _constant(name):
    with open(_SRC) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


CHUNK = _constant("QC")            # columns of sim / sim_q one workgroup of the queue loss kernels takes
THREADS = _constant("QT")          # threads of such a workgroup: each holds CHUNK / THREADS values in registers


def chunks(J, L):
    """(chunks of sim, chunks of sim_q) per row slot in the launcher's grid."""
    return (J + CHUNK - 1) // CHUNK, (L + CHUNK - 1) // CHUNK


def vectorised(J, L, *matrices):
    """True where the kernels move 16 bytes per lane, else 4: the launcher's condition, J % 4 == L % 4 == 0 and every one of
    sim, sim_q, dsim and dsim_q on a 16-byte address (`matrices`: the tensors handed to the entry)."""
    return J % 4 == 0 and L % 4 == 0 and all(m.data_ptr() % 16 == 0 for m in matrices)
