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

`SparseEmbeddingBag` is the pooled form (one row per bag of ids, `Table.lookup_bag` /
`Table.push_bag`), with the same conventions.
"""
import torch

__all__ = ["SparseEmbedding", "SparseEmbeddingBag"]


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
    docstring); `maximize` pushes the gradient itself instead of its negation.  On a table with
    admission on (`Table.set_admission`) a refused id reads as a zero row and its backward is
    skipped."""

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


class _LookupBag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, ids, offsets, weights, table, mode, scale):
        ctx.table, ctx.mode, ctx.scale = table, mode, scale
        ctx.save_for_backward(*((ids, offsets) if weights is None else (ids, offsets, weights)))
        return table.lookup_bag(ids, offsets, weights, mode, insert=True)

    @staticmethod
    def backward(ctx, grad):
        ids, offsets, *w = ctx.saved_tensors
        g = grad.contiguous()
        if g.dtype not in (torch.float32, torch.float64):
            raise TypeError("SparseEmbeddingBag takes float32 or float64 gradients, got %s" % g.dtype)
        ctx.table.push_bag(ids, offsets, g, w[0] if w else None, ctx.mode, scale=ctx.scale)
        return None, None, None, None, None, None, None


class SparseEmbeddingBag(torch.nn.Module):
    """`torch.nn.EmbeddingBag` over the HBM table: one pooled row per bag, [B, table.pull_elems],
    through `Table.lookup_bag(insert=True)`; no per-id tensor exists in either direction.

    forward(ids, offsets=None, per_sample_weights=None), int64 CUDA tensors:
      ids [B, L]  fixed-length bags, the id -1 is padding (not a member: it neither adds to the sum
                  nor counts in the mean); `offsets` must be None
      ids [n]     with torch's start offsets [B], or [B + 1] ending in n with include_last_offset
    mode "sum" or "mean"; per_sample_weights ([*ids.shape], sum only) scale each id's row.  Weights
    that require grad raise: their gradient is not computed.

    As `SparseEmbedding`: no torch parameters, the rows are updated by the table's push rule DURING
    `backward()` (`Table.push_bag` with scale -1, or +1 with `maximize`), every distinct id takes
    one step with its terms summed in fp64 in a defined order, so a backward pass is
    bit-reproducible; calling `backward()` twice on one graph applies two steps.  On a table with
    admission on (`Table.set_admission`) a refused id reads as a zero row (a member that still
    counts in the mean) and its backward is skipped."""

    def __init__(self, table, mode="sum", maximize=False, include_last_offset=False):
        super().__init__()
        if mode not in ("sum", "mean"):
            raise ValueError("mode is 'sum' or 'mean'")
        self.table, self.mode = table, mode
        self.maximize, self.include_last_offset = bool(maximize), bool(include_last_offset)
        self.register_buffer("_anchor", torch.zeros(()), persistent=False)

    def forward(self, ids, offsets=None, per_sample_weights=None):
        if ids.dtype != torch.int64:
            raise TypeError("ids must be int64")
        w = per_sample_weights
        if w is not None:
            if w.requires_grad:
                raise ValueError("per_sample_weights that require grad are not supported")
            if self.mode != "sum":
                raise ValueError("per_sample_weights need mode='sum'")
            if w.shape != ids.shape:
                raise ValueError("per_sample_weights must have the shape of ids")
        if ids.dim() == 2:
            if offsets is not None:
                raise ValueError("2-D ids are fixed-length bags: offsets must be None")
            B, L = ids.shape
            off = torch.arange(B + 1, dtype=torch.int64, device=ids.device) * L
        elif ids.dim() == 1:
            if offsets is None or offsets.dim() != 1 or offsets.dtype != torch.int64:
                raise ValueError("1-D ids need 1-D int64 offsets")
            off = offsets.to(ids.device)
            if not self.include_last_offset:
                off = torch.cat([off, torch.full((1,), ids.numel(), dtype=torch.int64, device=ids.device)])
        else:
            raise ValueError("ids must be 1-D or 2-D")
        anchor = self._anchor.detach().requires_grad_(torch.is_grad_enabled())
        return _LookupBag.apply(anchor, ids.contiguous().view(-1), off, None if w is None else w.detach(), self.table,
                                self.mode, 1.0 if self.maximize else -1.0)

    def extra_repr(self):
        return "pull_elems=%d, mode=%s, maximize=%s" % (self.table.pull_elems, self.mode, self.maximize)
