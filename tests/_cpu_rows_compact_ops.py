"""TEST SCAFFOLDING -- the row-compaction entry points (pn_rows_list, pn_rows_gather, pn_rows_scatter; csrc/pn_rows.hip) on the CPU
stand-in of tests/_cpu_rows_ops.py, by way of its dense-output and time-gradient layers so that every mode of a per-sample solve
runs with them.  The list is the product's own text run on host arrays (pn_rows_list_host); the two copies are torch indexing,
which moves values as bits."""
import torch

from pnode_amd import _lib

from _cpu_rows_tgrad_ops import CpuRowsTgradOps


class RowsCompactMixin(object):
    """What -pn_rows_compact 1 asks of a backend, for any CPU stand-in that has the other pn_rows_* methods."""
    rows_compact = True

    def rows_list(self, B, kind, src, idx, pos, count):
        self.calls["rows_list"] = self.calls.get("rows_list", 0) + 1
        assert src.is_contiguous() and idx.is_contiguous() and pos.is_contiguous() and src.numel() == idx.numel() == pos.numel() == B
        assert src.dtype == (torch.int32 if kind == 0 else torch.float64) and idx.dtype == pos.dtype == count.dtype == torch.int32
        _lib.check(_lib.load().pn_rows_list_host(B, kind, src.data_ptr(), idx.data_ptr(), pos.data_ptr(), count.data_ptr()))

    def rows_gather(self, m, d, out, src, idx):
        self.calls["rows_gather"] = self.calls.get("rows_gather", 0) + 1
        assert out.dtype == src.dtype and out.numel() >= m * d
        k = idx[:m].long()
        rows = src.detach().reshape(-1, d)[k.clamp(min=0)].clone()
        rows[k < 0] = 0
        out.detach()[: m * d].view(m, d).copy_(rows)

    def rows_scatter(self, B, d, out, src, pos):
        self.calls["rows_scatter"] = self.calls.get("rows_scatter", 0) + 1
        assert out.dtype == src.dtype and out.numel() >= B * d
        p = pos[:B].long()
        rows = torch.zeros(B, d, dtype=out.dtype)
        if src.numel():
            rows = src.detach().reshape(-1, d)[p.clamp(min=0)].clone()
            rows[p < 0] = 0
        out.detach()[: B * d].view(B, d).copy_(rows)


class CpuRowsCompactOps(RowsCompactMixin, CpuRowsTgradOps):
    pass
