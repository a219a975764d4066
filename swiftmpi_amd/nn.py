"""torch.nn front end of the HBM table: an embedding whose rows live in the parameter shard.

    table = swiftmpi_amd.Table("w2v", dim=64, capacity=1 << 20)
    emb = swiftmpi_amd.nn.SparseEmbedding(table)
    loss = model(emb(ids)).sum()
    loss.backward()            # the table's rows have been updated here

`SparseEmbedding` holds NO torch parameters and needs no torch optimiser: the optimiser step is
the server's push rule (AdaGrad, or SGD on an SGD table), applied by the table DURING
`backward()`, as a parameter server applies a worker's push.  Every distinct id of the batch
takes exactly one step with the fp64 sum of the gradients of its occurrences (the defined order
of `Table.push_dup`), so a backward pass is bit-reproducible.  The table's rule is ascent
(w += lr * g / sqrt(g2 + fudge)), so the backward pushes the NEGATED gradient; `maximize=True`
pushes it as it is.  An `optimizer.zero_grad()` / `step()` around it has nothing to do for this
module, and calling `backward()` twice on one graph applies two steps.
"""
import torch

__all__ = ["SparseEmbedding"]


class _Lookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, ids, table, scale):
        ctx.table, ctx.scale = table, scale
        ctx.save_for_backward(ids)
        pad = ids == -1
        if bool(pad.any()):  # padding ids read as zero rows; the inserting lookup takes real keys only
            out = torch.zeros((*ids.shape, table.pull_elems), dtype=table.torch_dtype, device=ids.device)
            out[~pad] = table.lookup(ids[~pad], insert=True)
            return out
        return table.lookup(ids, insert=True)

    @staticmethod
    def backward(ctx, grad):
        (ids,) = ctx.saved_tensors
        g = grad.contiguous()
        if g.dtype not in (torch.float32, torch.float64):
            raise TypeError("SparseEmbedding takes float32 or float64 gradients, got %s" % g.dtype)
        ctx.table.push_dup(ids, g, "sum", scale=ctx.scale)  # padding positions are skipped
        return None, None, None, None


class SparseEmbedding(torch.nn.Module):
    """forward(ids): an int64 CUDA tensor of any shape -> [*ids.shape, table.pull_elems] (W2V
    tables: [h | v], 2 * dim values; LR tables: the weight) through `Table.lookup(insert=True)`:
    ids the table lacks are inserted with its init rule.  The id -1 is padding: a zero row, no
    gradient.  The rows are updated by the table's push rule during `backward()` (see the module
    docstring); `maximize` pushes the gradient itself instead of its negation."""

    def __init__(self, table, maximize=False):
        super().__init__()
        self.table = table
        self.maximize = bool(maximize)
        # autograd only calls a Function's backward when an input requires grad: a constant anchor
        self.register_buffer("_anchor", torch.zeros(()), persistent=False)

    def forward(self, ids):
        if ids.dtype != torch.int64:
            raise TypeError("ids must be int64")
        anchor = self._anchor.detach().requires_grad_(torch.is_grad_enabled())
        return _Lookup.apply(anchor, ids, self.table, 1.0 if self.maximize else -1.0)

    def extra_repr(self):
        return "pull_elems=%d, maximize=%s" % (self.table.pull_elems, self.maximize)
