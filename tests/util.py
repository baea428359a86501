"""Shared helpers for the parity tests (layout conversion, error metrics)."""
import torch


def to_cn(x):
    """(B,C,T,V) -> CN matrix [C][B*T*V] (include/sar_hip.h)."""
    B, C, T, V = x.shape
    return x.permute(1, 0, 2, 3).reshape(C, B * T * V).contiguous()


def from_cn(y, B, T, V):
    C = y.shape[0]
    return y.reshape(C, B, T, V).permute(1, 0, 2, 3).contiguous()


def rel_err(a, b):
    """max |a-b| / max |b| (norm-wise relative error; b is the reference)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def rel_err_fro(a, b):
    """||a-b||_2 / ||b||_2 (Frobenius-relative error; b is the reference)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = b.norm().item()
    return (a - b).norm().item() / (denom if denom > 0 else 1.0)


# ---- bf16 (CN8) kernels: exact definitions shared by tests/test_gpu_cn8.py and tests/test_gpu_cn8_batch64.py

def bf(t):
    """the value a bf16 operand holds (round to nearest even), as float64"""
    return t.float().bfloat16().double()


def assert_bf16_close(got, ref, what=""):
    """a stored bf16 output: within one bfloat16 rounding (2^-8 relative per element) plus 1e-5 of the tensor scale for the
    accumulation order"""
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().item()
    bad = (got - ref).abs() - (2.0 ** -8) * ref.abs() - 1e-5 * scale
    assert bad.max().item() <= 0, "%s: worst excess %.3e (scale %.3e)" % (what, bad.max().item(), scale)


def graph_ref(x, kernel, bias, A, dev_tables):
    """exact definition: z_k = bf16(fp32 gather of the bf16 src in table order), W rounded to bf16, float64 contraction"""
    idx, wt = dev_tables.idx.cpu(), dev_tables.wt.cpu()                   # [3][V][4]
    Bq, cin, T, V = x.shape
    f = kernel.shape[3] // 3
    xs = x.float()
    out = torch.zeros(Bq, f, T, V, dtype=torch.float64)
    Wk = bf(kernel)[0, 0]                                                  # (cin, 3f)
    for k in range(3):
        z = torch.zeros(Bq, cin, T, V)
        for w in range(V):
            acc = None
            for j in range(dev_tables.nz[k]):
                term = wt[k, w, j] * xs[:, :, :, idx[k, w, j]]
                acc = term if acc is None else torch.addcmul(acc, xs[:, :, :, idx[k, w, j]], wt[k, w, j])   # fp32 fma chain
            z[:, :, :, w] = acc
        zb = bf(z)
        out += torch.einsum("bctv,cm->bmtv", zb, Wk[:, k * f:(k + 1) * f])
        if bias is not None:
            out += bias.double()[k * f:(k + 1) * f].view(1, -1, 1, 1) * A[k].double().sum(dim=0).view(1, 1, 1, -1)
    return out


# ---- guard bands: an operand as a view into a larger allocation whose every other element holds a known fill (tests/test_gpu_guard_bands.py)

NAN = float("nan")       # padding of inputs: whatever reads it and lets it reach a result shows
SENTINEL = -7.25         # padding of outputs (tests/test_gpu_graph_sample.py's poison value)
MASK_FILL = 0xA5         # padding of uint8 mask buffers


def _bits(t):
    """the bit patterns of a tensor (a NaN equals itself)"""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def guarded(src_or_shape, pad, fill, dev, front=4, back=2, dtype=torch.float32):
    """(view, whole): `whole` is ONE allocation of (front + C + back, n + pad) elements holding `fill`; view = whole[front:front + C, :n]
    holds `src` when a (C, n) tensor is given.  front = 4 rows keep the view's base 16-byte aligned for every leading dimension, so
    an odd `pad` changes only the alignment of the rows behind the first."""
    src = src_or_shape if torch.is_tensor(src_or_shape) else None
    C, n = src.shape if src is not None else src_or_shape
    whole = torch.full((front + C + back, n + pad), fill, dtype=dtype, device=dev)
    view = whole[front:front + C, :n]
    if src is not None:
        view.copy_(src)
    return view, whole


def guarded_flat(src_or_n, fill, dev, k=8, dtype=torch.float32):
    """(view, whole) of a 1-D range: k elements of `fill` in front of and behind the n live ones (k a multiple of 4: the view stays
    16-byte aligned)"""
    assert k % 4 == 0
    src = src_or_n if torch.is_tensor(src_or_n) else None
    n = src.numel() if src is not None else int(src_or_n)
    whole = torch.full((k + n + k,), fill, dtype=dtype, device=dev)
    view = whole[k:k + n]
    if src is not None:
        view.copy_(src.reshape(-1))
    return view, whole


def assert_guards_untouched(whole, view_shape, fill, front=4, back=2, what=""):
    """every element of `whole` outside whole[front:front + C, :n] still holds `fill`, bit for bit"""
    C, n = view_shape
    assert whole.dim() == 2 and whole.shape[0] == front + C + back and whole.shape[1] >= n, "%s: not a guarded allocation" % what
    want = _bits(torch.full((1,), fill, dtype=whole.dtype, device=whole.device))
    bad = _bits(whole) != want
    bad[front:front + C, :n] = False
    if bool(bad.any()):
        r, c = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: guard element (row %d, column %d) of a (%d, %d) view at row %d, ld %d was overwritten with %r (%d in all)"
                             % (what, r - front, c, C, n, front, whole.shape[1], whole[r, c].item(), int(bad.sum())))


def assert_flat_guards_untouched(whole, n, fill, k=8, what=""):
    assert whole.dim() == 1 and whole.numel() == n + 2 * k, "%s: not a guarded range" % what
    want = _bits(torch.full((1,), fill, dtype=whole.dtype, device=whole.device))
    bad = _bits(whole) != want
    bad[k:k + n] = False
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: guard element %d of a %d-element range was overwritten with %r (%d in all)"
                             % (what, i - k, n, whole[i].item(), int(bad.sum())))


# ---- one guarded launch and its five assertions (tests/test_gpu_guard_bands.py states them; tests/test_gpu_split_guard_bands.py
# runs the split-arithmetic kernels through the same ones)

def mask_bytes(keep):
    """(C, n) bool -> (C, n / 4) bytes, bit j = element 4 i + j (the mask layout of sar_bn_add_relu_fwd_f32)"""
    C, n = keep.shape
    return (keep.view(C, n // 4, 4).to(torch.int32) * torch.tensor([1, 2, 4, 8], dtype=torch.int32, device=keep.device)).sum(dim=2).to(torch.uint8)


class Launch:
    """the operands and results of one run of a case at one `pad`"""
    FRONT, BACK, KFLAT = 4, 2, 8      # guard rows of every operand, guard elements of a flat range
    IN_BACK = 2                       # guard rows behind an INPUT (a family whose stagers round the channel count up asks for more)

    KEEP_INPUTS = False               # keep a copy of every input's allocation: check() then asserts that no launch modified one

    def __init__(self, dev, pad):
        self.dev, self.pad = dev, pad
        self.outs, self.flats, self.masks, self.parts, self.refs, self.slabs = {}, {}, {}, {}, [], []
        self.ins, self.nan_ok = [], set()     # (name, allocation, its copy) of the kept inputs; outputs whose specified result holds NaN

    def inp(self, src):
        """a (C, n) input as a guarded view, NaN all around"""
        view, whole = guarded(src.float(), self.pad, NAN, self.dev, self.FRONT, self.IN_BACK)
        if self.KEEP_INPUTS:
            self.ins.append(("input %d" % len(self.ins), whole, whole.clone()))
        return view

    def flat_in(self, src, fill=NAN):
        """a flat input of src's dtype and shape between KFLAT elements of `fill` (an int64 label range takes a label no class has),
        kept: check() asserts that the live elements and both margins are what they were"""
        view, whole = guarded_flat(src, fill, self.dev, self.KFLAT, dtype=src.dtype)
        self.ins.append(("input %d" % len(self.ins), whole, whole.clone()))
        return view.view(src.shape)

    def check_inputs(self):
        for name, whole, copy in self.ins:
            bad = _bits(whole) != _bits(copy)
            assert not bool(bad.any()), "%s (pad %d): %d element(s) of an input's allocation were modified, the first at flat index %d" \
                % (name, self.pad, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))

    def out(self, name, C, n):
        view, whole = guarded((C, n), self.pad, SENTINEL, self.dev, self.FRONT, self.BACK)
        self.outs[name] = (view, whole)
        return view

    def flat(self, name, n):
        """a flat output of n elements, or an in-place buffer when a tensor is given (the live elements then start as its values)"""
        view, whole = guarded_flat(n, SENTINEL, self.dev, self.KFLAT)
        self.flats[name] = (view, whole)
        return view

    def mask(self, name, C, n, keep=None):
        """the (C, ld / 4) mask bytes of a (C, n) tensor of row stride ld = n + pad (ops.relu_mask's layout) with guard rows; the live
        bytes are columns [0, n / 4): from `keep` (C, n) bool when given.  Returns the contiguous (C, ld / 4) tensor the ABI takes."""
        whole = torch.full((self.FRONT + C + self.BACK, (n + self.pad) // 4), MASK_FILL, dtype=torch.uint8, device=self.dev)
        rows = whole[self.FRONT:self.FRONT + C]
        if keep is not None and n % 4 == 0:      # (rows that are no 4-element groups have no mask: the call is to be rejected)
            rows[:, :n // 4] = mask_bytes(keep).to(self.dev)
        self.masks[name] = (rows[:, :n // 4], whole)
        return rows

    def part(self, name, t, cols=None):
        """a reduction partial allocated inside ops: checked finite (cols: the leading entries of the last axis that are defined)"""
        self.parts[name] = t if cols is None else t[..., :cols]
        return t

    def slab_batch(self, reduce):
        """a GuardedSlabs for the `slabs=` of a weight-gradient call: its slabs are checked with the launch's other outputs"""
        self.slabs.append(GuardedSlabs(self.dev, reduce, self.KFLAT))
        return self.slabs[-1]

    def ref(self, what, got, want, tol, scale=None):
        """got (a device tensor or a callable evaluated after the launches) against `want`: rel_err < tol, or bitwise when tol == 0
        (scale: the error's denominator where a test states another one than max |want|)"""
        self.refs.append((what, got, want, tol, scale))

    def check(self):
        self.check_guards()                                                                      # 3
        self.check_inputs()
        for name, (view, _) in list(self.outs.items()) + list(self.flats.items()):                # 4
            assert name in self.nan_ok or bool(torch.isfinite(view).all()), "%s (pad %d): not finite" % (name, self.pad)
        for name, t in self.parts.items():
            assert bool(torch.isfinite(t).all()), "partials %s (pad %d): not finite" % (name, self.pad)
        for s in self.slabs:
            s.check_finite("slabs (pad %d)" % self.pad)
        for what, got, want, tol, scale in self.refs:                                            # 1
            got = got() if callable(got) else got
            want = want() if callable(want) else want
            if tol == 0:
                assert torch.equal(got.cpu(), want.cpu()), "%s (pad %d): not bitwise equal" % (what, self.pad)
            else:
                e = rel_err(got.cpu(), want.cpu()) if scale is None else (got.cpu().double() - want.cpu().double()).abs().max().item() / scale
                print("%s (pad %d): %.2e" % (what, self.pad, e))
                assert e < tol, "%s (pad %d): %.3e >= %.1e" % (what, self.pad, e, tol)

    def check_guards(self):
        for name, (view, whole) in self.outs.items():
            assert_guards_untouched(whole, view.shape, SENTINEL, self.FRONT, self.BACK, "%s (pad %d)" % (name, self.pad))
        for name, (view, whole) in self.masks.items():
            assert_guards_untouched(whole, view.shape, MASK_FILL, self.FRONT, self.BACK, "mask %s (pad %d)" % (name, self.pad))
        for name, (view, whole) in self.flats.items():
            assert_flat_guards_untouched(whole, view.numel(), SENTINEL, self.KFLAT, "%s (pad %d)" % (name, self.pad))
        for s in self.slabs:
            s.check_guards("slabs (pad %d)" % self.pad)

    def check_nothing_written(self):
        """5: a rejected call launched nothing"""
        for name, (_, whole) in list(self.outs.items()) + list(self.flats.items()):
            assert bool((whole == SENTINEL).all()), "%s (pad %d): written by a rejected call" % (name, self.pad)
        for s in self.slabs:
            s.check_nothing_written("slabs (pad %d)" % self.pad)


def drive(dev, fn, pad, bitwise=True, launch=Launch):
    """run `fn` tight and with `pad`, apply the five assertions"""
    tight, padded = launch(dev, 0), launch(dev, pad)
    fn(tight)
    fn(padded)
    torch.cuda.synchronize()
    tight.check()
    padded.check()
    # (a variant that a padded ld is rejected for has an output in the tight launch only)
    assert set(tight.outs) >= set(padded.outs) and set(tight.flats) == set(padded.flats) and set(tight.masks) >= set(padded.masks)
    if bitwise:                                                                                  # 2
        for kind in ("outs", "flats", "masks"):
            for name, (view, _) in getattr(padded, kind).items():
                assert torch.equal(view, getattr(tight, kind)[name][0]), "%s: pad %d differs from the tight launch" % (name, pad)
    return tight, padded


def rejected(dev, fn, pad, launch=Launch):
    """the ABI does not take this leading dimension: the call raises and writes nothing"""
    import pytest
    from sar_amd import _lib as L
    g = launch(dev, pad)
    with pytest.raises((L.SarError, AssertionError)):
        fn(g)
    torch.cuda.synchronize()
    g.check_nothing_written()


class GuardedSlabs:
    """What a weight-gradient call takes as `slabs=` (duck-typed to sar_amd.ops.SlabBatch: slab() and add()), with every slab a view
    into a guarded flat range: the live nsplit * n elements start as NaN -- an element no workgroup writes reaches the reduced
    gradient as NaN --, the KFLAT elements on either side hold the output sentinel.  add() reduces at once by `reduce(slab, nsplit,
    n, out)` (on the GPU: sar_slab_reduce_f32, the launch ops issues behind a weight gradient without a batch)."""

    def __init__(self, dev, reduce, k=8):
        self.dev, self.reduce, self.k, self.items = dev, reduce, k, []

    def slab(self, out, nsplit, n):
        view, whole = guarded_flat(nsplit * n, SENTINEL, self.dev, self.k)
        view.fill_(NAN)
        self.items.append((view, whole, nsplit, n))
        return view.view(nsplit, n)

    def add(self, slab, nsplit, n, out):
        assert any(slab.data_ptr() == v.data_ptr() and (nsplit, n) == (ns, nn) for v, _, ns, nn in self.items), "not a slab of this batch"
        self.reduce(slab, nsplit, n, out)

    def check_guards(self, what=""):
        for view, whole, nsplit, n in self.items:
            assert_flat_guards_untouched(whole, nsplit * n, SENTINEL, self.k, "%s: (%d, %d) slab" % (what, nsplit, n))

    def check_finite(self, what=""):
        assert self.items, "%s: the call asked for no slab" % what
        for view, _, nsplit, n in self.items:
            bad = ~torch.isfinite(view)
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                raise AssertionError("%s: element %d of slab %d of a (%d, %d) slab buffer was never written or is not finite (%d in all)"
                                     % (what, i % n, i // n, nsplit, n, int(bad.sum())))

    def check_nothing_written(self, what=""):
        for view, whole, nsplit, n in self.items:
            self.check_guards(what)
            assert bool(torch.isnan(view).all()), "%s: written by a rejected call" % what


# ---- guard bands of the bf16 (CN8) kernels: planes of 16-byte units (include/sar_hip.h "CN8"; tests/test_gpu_cn8_guard_bands.py)

def cn8_units(src):
    """(C, n) tensor of bf16-representable values -> (ceil(C/8), n, 8) bfloat16 on the host BY THE LAYOUT'S DEFINITION:
    unit (g, col)[j] = channel 8 g + j, zero for channels >= C (not through sar_cn_to_cn8, which is itself under test)"""
    C, n = src.shape
    G = (C + 7) // 8
    full = torch.zeros(G * 8, n, dtype=torch.float32)
    full[:C] = src.detach().float().cpu()
    assert torch.equal(full.bfloat16().float(), full), "cn8_units: values are not bfloat16-representable"
    return full.view(G, 8, n).permute(0, 2, 1).contiguous().bfloat16()


def cn8_values(units, C):
    """the inverse of cn8_units on the host: (G, n, 8) units -> (C, n) float32 (exact)"""
    G, n, _ = units.shape
    return units.detach().float().cpu().permute(0, 2, 1).reshape(G * 8, n)[:C].contiguous()


def guarded_cn8(src_or_shape, pad, fill, dev, front=2, back=2):
    """(view, whole): `whole` is ONE contiguous bf16 allocation of (front + G + back) planes x (n + pad) units x 8 holding `fill`,
    G = ceil(C/8); view = whole[front:front + G] is contiguous, of shape (G, ld = n + pad, 8): what ops8._cn8 accepts.  Given a
    (C, n) tensor, the live units view[:, :n] hold it (cn8_units: pad lanes zero, the ABI's contract for an input); given a
    shape (an output), the live units -- pad lanes included -- start as `fill`."""
    src = src_or_shape if torch.is_tensor(src_or_shape) else None
    C, n = src.shape if src is not None else src_or_shape
    G = (C + 7) // 8
    whole = torch.full((front + G + back, n + pad, 8), fill, dtype=torch.bfloat16, device=dev)
    view = whole[front:front + G]
    if src is not None:
        view[:, :n] = cn8_units(src).to(dev)
    return view, whole


def guarded_cn8_mask(src_or_shape, pad, dev, front=2, back=2):
    """(view, whole) of the CN8 mask layout -- one byte per unit, rows are planes: `whole` (front + G + back, n + pad) uint8 of
    MASK_FILL, view = whole[front:front + G] (contiguous, (G, ld)); the live bytes view[:, :n] from a (G, n) uint8 tensor if given"""
    src = src_or_shape if torch.is_tensor(src_or_shape) else None
    G, n = src.shape if src is not None else src_or_shape
    whole = torch.full((front + G + back, n + pad), MASK_FILL, dtype=torch.uint8, device=dev)
    view = whole[front:front + G]
    if src is not None:
        view[:, :n] = src.to(dev)
    return view, whole


def cn8_mask_bytes(keep):
    """(C, n) bool -> (ceil(C/8), n) bytes, bit j of byte (g, col) = channel 8 g + j (the mask layout of sar_bn_add_relu_fwd_cn8)"""
    C, n = keep.shape
    G = (C + 7) // 8
    kb = torch.zeros(G * 8, n, dtype=torch.int32)
    kb[:C] = keep.cpu().to(torch.int32)
    return (kb.view(G, 8, n) << torch.arange(8, dtype=torch.int32).view(1, 8, 1)).sum(dim=1).to(torch.uint8).contiguous()


def assert_cn8_guards_untouched(whole, C, n, fill, front=2, back=2, what=""):
    """every unit of `whole` outside planes [front, front + G) x columns [0, n) still holds `fill`, bit for bit"""
    G = (C + 7) // 8
    assert whole.dim() == 3 and whole.shape[0] == front + G + back and whole.shape[1] >= n and whole.shape[2] == 8, \
        "%s: not a guarded CN8 allocation" % what
    want = _bits(torch.full((1,), fill, dtype=whole.dtype, device=whole.device))
    bad = _bits(whole) != want
    bad[front:front + G, :n] = False
    if bool(bad.any()):
        g, c, j = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: guard unit (plane %d, column %d), lane %d of a (%d planes, %d columns) view at plane %d, ld %d was "
                             "overwritten with %r (%d elements in all)"
                             % (what, g - front, c, j, G, n, front, whole.shape[1], whole[g, c, j].item(), int(bad.sum())))


def assert_cn8_pad_lanes_zero(view, C, n, what=""):
    """lanes C % 8 .. 7 of the last plane's live units (the channels >= C) are zero: what every consumer assumes"""
    if C % 8 == 0:
        return
    lanes = view[(C + 7) // 8 - 1, :n, C % 8:]
    bad = _bits(lanes) & 0x7fff != 0                 # (+0 or -0)
    if bool(bad.any()):
        c, j = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: pad lane %d (channel %d >= %d) of column %d holds %r, not zero (%d in all)"
                             % (what, C % 8 + j, 8 * ((C + 7) // 8 - 1) + C % 8 + j, C, c, lanes[c, j].item(), int(bad.sum())))
