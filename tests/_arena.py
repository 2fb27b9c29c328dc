"""Guarded, poisoned device allocations for the memory-contract tests (a helper, no test).

include/kgat_hip.h promises that scratch is exactly what ``*_workspace_bytes`` answers, that outputs are fully
overwritten and that nothing depends on what a buffer held before the call.  ``guarded`` hands out a buffer of exactly
the bytes asked for between two 4,096-byte bands of a fixed pattern, its interior filled with a 32-bit poison word;
``patched`` puts such buffers behind every ``ops._workspace`` and every ``torch.empty`` / ``torch.empty_like`` the op
layer makes, records them, and records which C entries were called meanwhile."""
import contextlib

import torch

BAND = 4096
ALIGN = 256
_patterns = {}


def _pattern(device):
    """BAND bytes that are not all equal (and hold no run of four equal bytes): (37 i + 11) mod 251."""
    key = str(device)
    if key not in _patterns:
        _patterns[key] = ((torch.arange(BAND, dtype=torch.int64, device=device) * 37 + 11) % 251).to(torch.uint8)
    return _patterns[key]


def _signed32(word):
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word


class Guard:
    """One guarded allocation: `parent` keeps the memory alive, the interior is parent[off : off + nbytes]."""

    def __init__(self, nbytes, device, poison, what=""):
        self.nbytes, self.poison, self.what = int(nbytes), poison & 0xFFFFFFFF, what
        self.parent = torch.empty(BAND + ALIGN + self.nbytes + BAND, dtype=torch.uint8, device=device)
        base = self.parent.data_ptr()
        self.off = (base + BAND + ALIGN - 1) // ALIGN * ALIGN - base
        assert self.off >= BAND and self.off + self.nbytes + BAND <= self.parent.numel()
        pat = _pattern(device)
        self.parent[self.off - BAND:self.off] = pat
        self.parent[self.off + self.nbytes:self.off + self.nbytes + BAND] = pat
        self.bytes = self.parent[self.off:self.off + self.nbytes]
        assert self.bytes.data_ptr() % ALIGN == 0
        words = self.nbytes // 4
        if words:
            self.bytes[:4 * words].view(torch.int32).fill_(_signed32(self.poison))
        for i in range(4 * words, self.nbytes):
            self.bytes[i] = (self.poison >> (8 * (i % 4))) & 0xFF

    def tensor(self, shape, dtype):
        return self.bytes.view(dtype).view(shape)

    def bands_intact(self):
        """(before, after) - call after torch.cuda.synchronize()."""
        pat = _pattern(self.parent.device)
        return (bool(torch.equal(self.parent[self.off - BAND:self.off], pat)),
                bool(torch.equal(self.parent[self.off + self.nbytes:self.off + self.nbytes + BAND], pat)))

    def poison_words(self):
        """Bool mask over the interior's whole 32-bit words: True where the word still is the poison."""
        return poison_words(self.bytes, self.poison)


def poison_words(t, poison):
    """Bool mask over the 32-bit words of `t`'s elements in row-major order (any dtype, any strides)."""
    flat = t.contiguous().view(-1).view(torch.uint8)
    words = flat.numel() // 4
    return flat[:4 * words].view(torch.int32) == _signed32(poison)


def guarded(nbytes, device, poison):
    """A contiguous uint8 tensor of exactly `nbytes` bytes on a 256-byte boundary, between two guard bands, filled
    with the word `poison`; its Guard (bands_intact, poison_words) is the tensor's attribute `guard`."""
    g = Guard(nbytes, device, poison, "guarded")
    t = g.bytes
    t.guard = g
    return t


class _TorchProxy:
    """`torch` as the op layer sees it inside `patched`: everything forwarded, device `empty` / `empty_like` guarded."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dev = torch.device(device) if device is not None else None
        if dev is None or dev.type != "cuda":
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        assert not kw, "a device torch.empty with %s would escape the arena: guard it here first" % sorted(kw)
        return self._arena.empty(shape, dtype or torch.get_default_dtype(), dev, "torch.empty")

    def empty_like(self, t, dtype=None, **kw):
        if not t.is_cuda:
            return torch.empty_like(t, dtype=dtype, **kw)
        assert not kw, "a device torch.empty_like with %s would escape the arena: guard it here first" % sorted(kw)
        return self._arena.empty(tuple(t.shape), dtype or t.dtype, t.device, "torch.empty_like")


class _LibSpy:
    """The loaded library with every call of a kgat_* entry noted in `calls`."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("kgat_"):
            return fn

        def call(*args):
            self._calls.append(name)
            return fn(*args)
        return call


class Arena:
    def __init__(self, poison):
        self.poison = poison & 0xFFFFFFFF
        self.guards = []     # every guarded allocation handed out, in order
        self.calls = []      # names of the C entries called while patched

    def empty(self, shape, dtype, device, what="test"):
        n = 1
        for s in shape:
            n *= int(s)
        if n == 0:           # nothing to guard, and nothing a kernel may touch
            return torch.empty(shape, dtype=dtype, device=device)
        g = Guard(n * dtype.itemsize, device, self.poison, "%s%s %s" % (what, shape, dtype))
        self.guards.append(g)
        return g.tensor(shape, dtype)

    def workspace(self, nbytes, device):
        """ops._workspace with exactly the bytes the size function answered (256 only where it answered 0)."""
        nbytes = int(nbytes)
        g = Guard(nbytes if nbytes > 0 else 256, device, self.poison, "workspace of %d bytes" % nbytes)
        self.guards.append(g)
        return g.bytes

    def broken_bands(self):
        """The allocations with a damaged band, as text - after torch.cuda.synchronize()."""
        bad = []
        for g in self.guards:
            before, after = g.bands_intact()
            if not (before and after):
                bad.append("%s: band %s written" % (g.what, "before and after" if not (before or after) else
                                                    "before" if not before else "after"))
        return bad


@contextlib.contextmanager
def patched(ops, poison, scratch_only=False):
    """For its duration: `ops._workspace` is a guarded buffer of exactly the bytes asked for, the name `torch` inside
    the `ops` module is a proxy whose device `empty` / `empty_like` are guarded and poisoned (not with scratch_only:
    then only the workspaces are replaced), and the calls of C entries are noted.  Yields the Arena."""
    from dgl_kgat_amd import _lib
    arena = Arena(poison)
    lib = _lib.load()
    saved = (ops._workspace, ops.torch, _lib._lib)
    try:
        ops._workspace = arena.workspace
        if not scratch_only:
            ops.torch = _TorchProxy(arena)
        _lib._lib = _LibSpy(lib, arena.calls)
        yield arena
    finally:
        ops._workspace, ops.torch, _lib._lib = saved
