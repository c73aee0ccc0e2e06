"""wsa_gather: the rows of several GPUs' batches on one device."""
import ctypes

import numpy as np

from ._abi import NFEAT, WsaError
from ._util import _Handle


class _GatherResult(ctypes.Structure):
    _fields_ = [("n_ranks", ctypes.c_uint32), ("n_rows", ctypes.c_uint32), ("rows_per_rank", ctypes.POINTER(ctypes.c_uint32)),
                ("d_row_meta", ctypes.c_void_p), ("d_row_feat", ctypes.c_void_p)]


class Gather(_Handle):
    """wsa_gather: the feature rows of the batches of several contexts (one per GPU, this process) collected on the root's device
    with one grouped RCCL exchange (include/wsa.h)."""

    _destroy = "wsa_gather_destroy"

    def __init__(self, analyzers, root=0):
        self.L = analyzers[0].L
        self.ans = list(analyzers)
        self.h = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(self.ans))(*[a.h for a in self.ans])
        st = self.L.wsa_gather_create(arr, len(self.ans), int(root), ctypes.byref(self.h))
        if st != 0:
            raise WsaError(f"wsa_gather_create failed ({st}): {self.L.wsa_last_error(self.ans[root].h).decode()}")
        self.root = root

    def rows(self, batches, streams=None):
        """-> (rows_per_rank, meta [n, 8] i32, feat [n, 53] f64) on the host, rank after rank"""
        n = len(self.ans)
        ba = (ctypes.c_void_p * n)(*[b.h for b in batches])
        sa = (ctypes.c_void_p * n)(*[int(s) for s in streams]) if streams is not None else None
        r = _GatherResult()
        self.ans[self.root]._check(self.L.wsa_gather_rows(self.h, ba, sa, ctypes.byref(r)))
        per = [int(r.rows_per_rank[i]) for i in range(n)]
        meta = np.zeros((r.n_rows, 8), np.int32)
        feat = np.zeros((r.n_rows, NFEAT), np.float64)
        self.ans[self.root]._check(self.L.wsa_gather_copy_rows(self.h, meta.ctypes.data, feat.ctypes.data, max(int(r.n_rows), 1)))
        return per, meta, feat
