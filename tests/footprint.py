"""Memory-footprint harness: every device tensor a test or the package creates sits between two guard bands.

    with Footprint("cuda", fill=POISON) as fp:
        x = fp.place(host_tensor)              # [band | payload | band], payload 512-byte aligned
        out = ops.some_kernel(x)               # torch.empty(..., device=...) inside ops.py is intercepted as well
    # leaving the block synchronises and checks every band bit for bit (FootprintError names tensor, call site, side, offset)

  * bands are bytes 0xFF: NaN as fp32 and as bf16, 255 as uint8, -1 as an integer.  A read past a tensor that reaches a result shows up
    in the value comparison of the test; a write past it in the exit check.
  * the payload of an ``empty*`` call is filled with ``fill``: POISON (0xFF) or CLEAN (0x00).  A result that differs between the two
    fills depends on memory nobody wrote.  ``zeros`` / ``full`` / ``ones`` / copies keep their defined contents.
  * each band is max(64 KiB, one plane of the tensor = H * row_stride * itemsize) rounded up to 512 bytes: a condition, not a
    measurement -- any vector store, any tile of rows and a one-plane stride error at the shapes of the suite stay inside it.

Only attributes of ``torch`` are patched, for the duration of the block: the creator functions (``empty``, ``empty_like``,
``empty_strided``, ``zeros``, ``zeros_like``, ``ones``, ``ones_like``, ``full``, ``full_like``, ``tensor``) where they name the device,
``Tensor.cuda`` / ``Tensor.to`` of a host tensor, and the device-side copies the tests build operands with (``Tensor.to(dtype)``,
``contiguous``, ``clone``, ``float``, ``bfloat16``).  Tensors that take part in autograd pass through untouched."""
import sys

import torch

POISON, CLEAN = 0xFF, 0x00
BAND_MIN = 64 * 1024
ALIGN = 512

_CREATORS = ("empty", "zeros", "ones", "full", "empty_strided")
_LIKES = ("empty_like", "zeros_like", "ones_like", "full_like")
_COPIES = ("contiguous", "clone", "float", "bfloat16")          # Tensor methods whose fresh result on the device is re-homed between bands
_HERE = __file__.rsplit(".", 1)[0]


class FootprintError(AssertionError):
    pass


def band_bytes(size, stride, itemsize):
    """max(64 KiB, H * row_stride * itemsize) rounded up to 512; tensors of fewer than two dimensions count as one plane"""
    if len(size) >= 2:
        plane = int(size[-2]) * int(stride[-2]) * itemsize
    else:
        plane = (int(size[0]) * int(stride[0]) if len(size) else 1) * itemsize
    return -(-max(BAND_MIN, plane) // ALIGN) * ALIGN


class _Record:
    __slots__ = ("raw", "lo", "hi", "shape", "dtype", "site", "what")

    def __init__(self, raw, lo, hi, shape, dtype, site, what):
        self.raw, self.lo, self.hi, self.shape, self.dtype, self.site, self.what = raw, lo, hi, shape, dtype, site, what


def _site():
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename.rsplit(".", 1)[0] == _HERE:
        f = f.f_back
    return "?" if f is None else f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"


class Footprint:
    def __init__(self, device="cuda", fill=POISON):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.fill = int(fill)
        self.records = []
        self._orig = {n: getattr(torch, n) for n in _CREATORS + _LIKES}
        self._orig_tensor = torch.tensor
        self._orig_cuda, self._orig_to = torch.Tensor.cuda, torch.Tensor.to
        self._orig_m = {n: getattr(torch.Tensor, n) for n in _COPIES}
        self._active = False

    # ---- the guarded allocation ----------------------------------------------------------------------------------------------
    @property
    def guarded(self):
        """number of guarded allocations so far"""
        return len(self.records)

    def _mine(self, device):
        if device is None:
            return False
        d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def alloc(self, size, dtype=torch.float32, stride=None, fill=None, what="alloc", site=None):
        """a tensor of the given size / stride between two bands; the payload (every byte of the storage extent) holds ``fill``"""
        size = tuple(int(s) for s in (size if isinstance(size, (tuple, list, torch.Size)) else (size,)))
        if stride is None:
            stride = tuple(self._orig["empty"](size, device="meta").stride())
        stride = tuple(int(s) for s in stride)
        item = torch.empty((), dtype=dtype, device="meta").element_size()
        extent = 0 if any(s == 0 for s in size) else 1 + sum((n - 1) * st for n, st in zip(size, stride))
        nbytes = extent * item
        band = band_bytes(size, stride, item)
        raw = self._orig["empty"](band + nbytes + band + ALIGN, dtype=torch.uint8, device=self.device)
        lo = band + (-(raw.data_ptr() + band)) % ALIGN
        hi = lo + nbytes
        raw.fill_(0xFF)
        fill = self.fill if fill is None else int(fill)
        if nbytes and fill != 0xFF:
            raw[lo:hi].fill_(fill)
        t = raw[lo:hi].view(dtype).as_strided(size, stride)
        assert nbytes == 0 or t.data_ptr() % ALIGN == 0
        self.records.append(_Record(raw, lo, hi, size, dtype, site or _site(), what))
        return t

    def place(self, t, fill=None):
        """a copy of ``t`` (same shape, dtype and strides; a view of a wider buffer keeps its pad elements, filled with ``fill``)
        on the harness device between two bands"""
        if t is None:
            return None
        out = self.alloc(t.shape, t.dtype, t.stride(), fill=fill, what="place", site=_site())
        with torch.no_grad():
            out.copy_(t)
        return out

    # ---- interception --------------------------------------------------------------------------------------------------------
    def _like_meta(self, meta, kwargs, what, site):
        out = self.alloc(meta.shape, meta.dtype, meta.stride(), what=what, site=site)
        return out.requires_grad_(True) if kwargs.get("requires_grad") else out

    def _wrap_creator(self, name):
        orig = self._orig[name]
        like = name.endswith("_like")

        def creator(*args, **kwargs):
            device = kwargs.get("device")
            if like and device is None and args and isinstance(args[0], torch.Tensor):
                device = args[0].device
            plain = kwargs.get("out") is None and not kwargs.get("pin_memory") and kwargs.get("layout", torch.strided) is torch.strided
            if not (self._active and plain and self._mine(device)):
                return orig(*args, **kwargs)
            meta = orig(*args, **{**kwargs, "device": "meta", "requires_grad": False})
            out = self._like_meta(meta, {}, "torch." + name, _site())
            with torch.no_grad():
                if name.startswith("zeros"):
                    out.zero_()
                elif name.startswith("ones"):
                    out.fill_(1)
                elif name.startswith("full"):
                    out.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[1])
            return out.requires_grad_(True) if kwargs.get("requires_grad") else out

        creator.__name__ = name
        return creator

    def _copy_in(self, src, dtype, non_blocking, memory_format, what):
        if dtype is not None and dtype != src.dtype:
            src = self._orig_to(src, dtype)
        if memory_format is not None and memory_format != torch.preserve_format:
            src = self._orig_m["contiguous"](src, memory_format=memory_format)
        meta = self._orig["empty_like"](src, device="meta")
        out = self.alloc(meta.shape, meta.dtype, meta.stride(), what=what, site=_site())
        out.copy_(src, non_blocking=bool(non_blocking))
        return out

    def _takes(self, t, device):
        return (self._active and self._mine(device) and t.device.type == "cpu" and not t.requires_grad and t.layout is torch.strided
                and not t.is_quantized)

    def _cuda(self, t, *args, **kwargs):
        device = kwargs.get("device", args[0] if args else None)
        if self.device.type != "cuda" or not self._takes(t, "cuda" if device is None else device):
            return self._orig_cuda(t, *args, **kwargs)
        nb = kwargs.get("non_blocking", args[1] if len(args) > 1 else False)
        return self._copy_in(t, None, nb, kwargs.get("memory_format"), "Tensor.cuda")

    def _to(self, t, *args, **kwargs):
        try:
            device, dtype, nb, mf = torch._C._nn._parse_to(*args, **kwargs)
        except Exception:
            return self._orig_to(t, *args, **kwargs)
        if device is None or not self._takes(t, device):
            return self._rehome(t, self._orig_to(t, *args, **kwargs), "Tensor.to")
        return self._copy_in(t, dtype, nb, mf, "Tensor.to")

    def _rehome(self, t, r, what):
        """a fresh tensor that a device-side copy (dtype change, layout change, clone) returned: the same values between bands"""
        if not (self._active and isinstance(r, torch.Tensor) and r is not t and r._base is None and self._mine(r.device)
                and not r.requires_grad and r.layout is torch.strided and not r.is_quantized):
            return r
        out = self.alloc(r.shape, r.dtype, r.stride(), what=what, site=_site())
        out.copy_(r)
        return out

    def _wrap_method(self, name):
        orig = self._orig_m[name]
        return lambda t, *a, **k: self._rehome(t, orig(t, *a, **k), "Tensor." + name)

    def _tensor(self, *args, **kwargs):
        device = kwargs.get("device")
        if not (self._active and self._mine(device)) or kwargs.get("pin_memory"):
            return self._orig_tensor(*args, **kwargs)
        host = self._orig_tensor(*args, **{**kwargs, "device": "cpu", "requires_grad": False})
        out = self._copy_in(host, None, False, None, "torch.tensor")
        return out.requires_grad_(True) if kwargs.get("requires_grad") else out

    # ---- context -------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        self._had = {n: n in torch.Tensor.__dict__ for n in ("cuda", "to") + _COPIES}
        for n in self._orig:
            setattr(torch, n, self._wrap_creator(n))
        me = self
        torch.tensor = lambda *a, **k: me._tensor(*a, **k)
        for n in _COPIES:
            setattr(torch.Tensor, n, self._wrap_method(n))
        torch.Tensor.cuda = lambda t, *a, **k: me._cuda(t, *a, **k)
        torch.Tensor.to = lambda t, *a, **k: me._to(t, *a, **k)
        self._active = True
        return self

    def _restore(self):
        self._active = False
        for n, f in self._orig.items():
            setattr(torch, n, f)
        torch.tensor = self._orig_tensor
        for n, f in (("cuda", self._orig_cuda), ("to", self._orig_to)) + tuple(self._orig_m.items()):
            if self._had[n]:
                setattr(torch.Tensor, n, f)
            elif n in torch.Tensor.__dict__:
                delattr(torch.Tensor, n)

    def __exit__(self, exc_type, exc, tb):
        self._restore()
        if exc_type is None:
            self.check()
        return False

    def check(self):
        """synchronise and compare every band with 0xFF, bit for bit"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self.records:
            return
        counts = torch.stack([torch.stack([(r.raw[:r.lo] != 0xFF).sum(), (r.raw[r.hi:] != 0xFF).sum()]) for r in self.records]).cpu()
        msgs = []
        for r, (before, after) in zip(self.records, counts.tolist()):
            for side, n, region, base in (("before", before, r.raw[:r.lo], r.lo), ("after", after, r.raw[r.hi:], 0)):
                if n:
                    first = int((region != 0xFF).nonzero()[0].item())
                    msgs.append(f"{r.what} of shape {tuple(r.shape)} {r.dtype} created at {r.site}: band {side} the payload damaged, "
                                f"{n} byte(s), first at offset {first - base:+d} from the payload's "
                                f"{'start' if side == 'before' else 'end'} (payload {r.hi - r.lo} bytes)")
        if msgs:
            raise FootprintError("memory written outside a tensor:\n  " + "\n  ".join(msgs))


def differing(a, b):
    """bit-level inequality of two tensors of one shape and dtype (NaN payloads included)"""
    if a.dtype.is_floating_point:
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.contiguous().view(it) != b.contiguous().view(it)
    return a != b


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and not bool(differing(a, b).any())
