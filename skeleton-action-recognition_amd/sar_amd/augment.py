"""Training-time augmentation of skeleton clips on the device: the host draws 16 numbers per clip, csrc/augment.hip applies them
(ops.augment_clips; the transform itself is stated in DESIGN.md "Augmentation" and restated in tests/augment_reference.py).

A parameter row is  [p, o, alpha0, beta0, gamma0, s0, dx0, dy0, dz0, alpha1, beta1, gamma1, s1, dx1, dy1, dz1]:
  p, o            the temporal crop keeps floor(p L) of the clip's L valid frames, starting at floor(o (L - Lc + 1))
  alpha..gamma    rotation about x, y, z in radians (R = Rz Ry Rx about the origin), s the scale, d the shift -- once for the first
                  output frame (index 0) and once for the last (index 1); the frames between move linearly from one to the other
                  (ST-GCN's `random_move`; `move=False` makes both key frames equal: 2s-AGCN / CTR-GCN's `random_rot`)

The table of a step is a function of (seed, epoch, iteration, rank) alone: it is drawn from
np.random.Generator(np.random.Philox(key=seed, counter=[epoch, iteration, rank, 0])) by ONE call u = random((n, 16)) (float64,
uniform in [0, 1)), column j of u making column j of the table:
  p = crop + (1 - crop) u      o = u      angle = rot (2 u - 1)      s = 1 + scale (2 u - 1)      d = shift (2 u - 1)
then rounded to float32 (o may round to 1.0; the kernel's min() covers it).  All 16 numbers are always drawn, so switching one
component on or off does not move the others; a component whose range is 0 (crop=None for p, o) holds its neutral value exactly:
p = 1, o = 0, angle = 0, s = 1, d = 0.  A resumed run, a re-run and a run on another machine draw the same tables."""
import numpy as np

NEUTRAL = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
_KEYS = ("rot", "scale", "shift", "crop", "move")


class ClipAugment:
    def __init__(self, rot=0.0, scale=0.0, shift=0.0, crop=None, move=True, seed=0):
        rot, scale, shift = float(rot), float(scale), float(shift)
        if not (np.isfinite(rot) and rot >= 0):
            raise ValueError("augment: rot must be a finite angle >= 0 (radians), got %r" % rot)
        if not (0 <= scale < 1):
            raise ValueError("augment: scale must lie in [0, 1), got %r" % scale)
        if not (np.isfinite(shift) and shift >= 0):
            raise ValueError("augment: shift must be finite and >= 0, got %r" % shift)
        if crop is not None:
            crop = float(crop)
            if not (0 < crop <= 1):
                raise ValueError("augment: crop must lie in (0, 1], got %r" % crop)
        if int(seed) < 0:
            raise ValueError("augment: seed must be >= 0, got %r" % seed)
        self.rot, self.scale, self.shift, self.crop, self.move, self.seed = rot, scale, shift, crop, bool(move), int(seed)
        key = [rot, rot, rot, scale, shift, shift, shift]
        self._range = np.array([0.0, 0.0] + key + key)         # p and o are drawn on their own (table)

    @classmethod
    def parse(cls, spec, seed=0):
        """'rot=0.3,scale=0.1,shift=0.1,crop=0.5,move=1' -> ClipAugment; unknown keys and values out of range raise ValueError"""
        kw = {}
        for item in str(spec).split(","):
            key, eq, val = item.strip().partition("=")
            if key not in _KEYS or not eq or key in kw:
                raise ValueError("augment: cannot read %r (keys: %s, each once, as key=value)" % (item, ", ".join(_KEYS)))
            if key == "move":
                if val not in ("0", "1"):
                    raise ValueError("augment: move must be 0 or 1, got %r" % val)
                kw[key] = val == "1"
            else:
                try:
                    kw[key] = float(val)
                except ValueError:
                    raise ValueError("augment: %s needs a number, got %r" % (key, val)) from None
        return cls(seed=seed, **kw)

    def table(self, n, epoch, iteration, rank=0):
        """the (n, 16) float32 parameter rows of step (epoch, iteration) on `rank`"""
        g = np.random.Generator(np.random.Philox(key=self.seed, counter=[int(epoch), int(iteration), int(rank), 0]))
        u = g.random((int(n), 16))
        # neutral + range * (2 u - 1), all columns at once; a range of 0 leaves the neutral value exactly (x + -0.0 is x, 0.0 + -0.0 is 0.0)
        tab = NEUTRAL + self._range * (2.0 * u - 1.0)
        if self.crop is not None:
            tab[:, 0] = self.crop + (1.0 - self.crop) * u[:, 0]
            tab[:, 1] = u[:, 1]
        if not self.move:
            tab[:, 9:16] = tab[:, 2:9]
        return tab.astype(np.float32)

    def __call__(self, x, epoch, iteration, rank=0, out=None):
        """the augmented batch of x (N, 3, T, V, M) on x's device: the table goes through a pinned buffer and a non-blocking copy on
        the current stream, then one launch; the host never waits for the device"""
        import torch
        from . import ops
        tab = self.table(x.shape[0], epoch, iteration, rank)
        # a fresh block of torch's pinned-memory cache per step: the cache hands a block out again only after the copy that read
        # it has finished on its stream, so the next step's table cannot overwrite one still in flight
        staged = torch.empty(tab.shape, dtype=torch.float32, pin_memory=True)
        staged.numpy()[:] = tab
        return ops.augment_clips(x, staged.to(x.device, non_blocking=True), crop=self.crop is not None, out=out)
