"""What the training engines share on the host: parameters as views of ONE flat fp32 buffer, the weight-gradient stream and the
third stream with their fork / join discipline, the gradient buckets of the data-parallel exchange.  sar_amd/stgcn.py (and its
siblings) and sar_amd/resnet.py derive from FlatEngine; an engine declares `shapes`, `bn` and `_buckets` and brings its own
_view() / _make_buckets()."""
import numpy as np
import torch

from . import ops


class FlatEngine:
    moving_suffixes = (".moving_mean", ".moving_var")      # a BatchNorm's moving statistics in load_params() / state_dict()

    # ------------------------------------------------------------------ flat storage
    def _allocate_flat(self, state, scalars=()):
        """self.shapes (insertion order) -> offsets, flat, grad, the views p / g, the device-side learning rate, and the optimizer's
        `state` buffers (as long as flat) and `scalars` (one element).  Every offset is a multiple of 4 floats so that each weight
        view is 16-byte aligned (the GEMM kernels stage weight rows as float4); a ".kernel" has a multiple of 4 elements, so its
        bias stays glued to it: the weight-gradient slabs are reduced as one contiguous [kernel | bias] range.  Returns the
        buffers' length."""
        total, self.offsets = 0, {}
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            assert n % 4 == 0 or not k.endswith(".kernel"), k
            self.offsets[k] = total
            total += (n + 3) // 4 * 4
        self.n_params = sum(int(np.prod(shp)) for shp in self.shapes.values())
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
        self.flat, self.grad, self.lr_dev = z(total), z(total), z(1)
        for name in state:
            setattr(self, name, z(total))
        for name in scalars:
            setattr(self, name, z(1))
        self._lr_host = None      # the value lr_dev holds; None = unknown
        self.p = {k: self._view(self.flat, k) for k in self.shapes}
        self.g = {k: self._view(self.grad, k) for k in self.shapes}
        return total

    def _view(self, flat, name):
        o = self.offsets[name]
        return flat[o:o + int(np.prod(self.shapes[name]))].view(self.shapes[name])

    def _set_lr(self, lr):
        if self._lr_host != float(lr):      # one launch less per step while the schedule holds the rate
            self.lr_dev.fill_(float(lr))
            self._lr_host = float(lr)

    def load_params(self, params):
        """params: dict name -> tensor in the layouts of self.shapes (incl. optional moving statistics; other keys ignored)"""
        mean, var = self.moving_suffixes
        for k, v in params.items():
            if k in self.p:
                self.p[k].copy_(v.to(torch.float32).reshape(self.shapes[k]))
            elif k.endswith(mean):
                self.bn[k[:-len(mean)]].moving_mean.copy_(v.to(torch.float32))
            elif k.endswith(var):
                self.bn[k[:-len(var)]].moving_var.copy_(v.to(torch.float32))

    def state_dict(self):
        mean, var = self.moving_suffixes
        out = {k: v.detach().cpu().clone() for k, v in self.p.items()}
        for k, b in self.bn.items():
            out[k + mean] = b.moving_mean.cpu().clone()
            out[k + var] = b.moving_var.cpu().clone()
        return out

    # ------------------------------------------------------------------ streams
    def _init_streams(self, side_priority, slab_batch, third_stream):
        """side_priority: priority of the weight-gradient stream (torch convention: lower = more urgent), None = no such stream;
        slab_batch: one slab reduction per gradient bucket (ops.SlabBatch) instead of one per weight gradient; third_stream: the
        stream of _fork().  No streams on a CPU device.  The helpers below read self._side / self._aux when they are called: a
        caller may set either to None on a live engine and put it back."""
        cuda = self.device.type == "cuda"
        self._side = ops.shared_side_stream(self.device, side_priority) if (cuda and side_priority is not None) else None
        self._slabs = ops.SlabBatch() if slab_batch else None
        self._slab_flush = ops.SLAB_FLUSH
        self._aux = ops.shared_aux_stream(self.device) if (cuda and third_stream) else None
        self._bounds_forked = False

    def _on_side(self, fn, *tensors):
        """fn() on the weight-gradient stream, ordered after everything issued so far: weight-gradient kernels feed nothing but the
        optimizer, so the MFMA-bound reductions overlap the HBM-bound BatchNorm / ReLU passes of the main chain.  `tensors` are the
        inputs whose memory the caching allocator must not hand out again before that stream is done with them.  On by default
        (SAR_WGRAD_STREAM=0 turns it off): measured +3.5 % clips/s at bs = 64 in fp32 -- the MFMA kernels fill the register file,
        so only part of the element-wise work can co-reside.  Per-kernel timings of overlapping kernels are inflated; bench.py
        therefore also reports the dominant family measured in a short pass with the side stream off (roofline.isolated)."""
        if self._side is None:
            fn()
            return
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            fn()
        for t in tensors:
            if t is not None:
                t.record_stream(self._side)

    def _fork(self, fn, *tensors, after="main"):
        """fn() on the third stream, ordered behind the current stream (after="main"), behind the event `after` only -- the fork may then
        start before the current stream's later launches -- or, after="nothing", behind the third stream's own work alone (anything
        else, None included, fails in wait_event); `tensors` as for _on_side.  _join() is where the main chain needs the results.
        Without the stream: fn() in place."""
        if self._aux is None:
            fn()
            return
        if after == "main":
            self._aux.wait_stream(torch.cuda.current_stream())
        elif after != "nothing":
            self._aux.wait_event(after)
        with torch.cuda.stream(self._aux):
            fn()
        for t in tensors:
            t.record_stream(self._aux)

    def _join(self):
        if self._aux is not None:
            torch.cuda.current_stream().wait_stream(self._aux)

    # ------------------------------------------------------------------ gradient buckets (data-parallel exchange)
    # self._buckets: contiguous slices of the flat gradient buffer in the order backward() completes them, each (block index after
    # whose backward the slice is complete, or -1 = at the end of backward; lo; hi)
    def _flush_slabs(self):
        """the slabs of every weight gradient issued since the last flush are summed by ONE launch on the weight-gradient stream
        (ops.SlabBatch): before a bucket is handed to the all-reduce and at the end of backward()"""
        if self._slabs is None:
            return
        if self._side is None:
            self._slabs.flush()
        else:
            with torch.cuda.stream(self._side):
                self._slabs.flush()

    def _bucket_done(self, bi, cb):
        """Every gradient of bucket bi has been ISSUED: weight gradients on the side stream, BatchNorm / bias gradients on the
        main stream.  cb(bi, flat slice, events) may start the slice's all-reduce once the events have completed -- the main stream
        goes on with the earlier layers."""
        _, lo, hi = self._buckets[bi]
        events = []
        self._flush_slabs()
        if self._side is not None:
            ev = torch.cuda.Event()
            ev.record(self._side)
            events.append(ev)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        events.append(ev)
        cb(bi, self.grad[lo:hi], events)

    def _buckets_after_block(self, i, cb):
        if cb is not None:
            for bi, (blk, _, _) in enumerate(self._buckets):
                if blk == i:
                    self._bucket_done(bi, cb)
        elif self._slabs is not None and (
                self._slab_flush == "block" or (self._slab_flush == "bucket" and any(blk == i for blk, _, _ in self._buckets))):
            self._flush_slabs()      # (experiment switch SAR_SLAB_FLUSH: more, smaller slab reductions than one at the end of backward)

    def _finish_backward(self, cb):
        """common tail of backward(): the remaining buckets go, the slabs are summed, the side stream is joined"""
        if cb is not None:
            self._buckets_after_block(-1, cb)
        self._flush_slabs()
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)      # every weight gradient is in self.grad
        self._saved = None
