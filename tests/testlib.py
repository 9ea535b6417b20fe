"""What the test modules share and no reference owns: the library fixtures, the status codes of include/golhip.h
as literals (the independent pin of the ABI; tests/test_testlib_cpu.py holds them against golhip._lib and the
header), the reader of the device error word, and Guarded, the one device buffer between two poisoned margins
that makes a kernel's out-of-place write visible.  A test module takes the fixture it needs under the name its
tests ask for: `from testlib import gpu_lib as G`, `from testlib import cpu_lib as G`, `from testlib import env`."""
import ctypes
import os
import types

import numpy as np
import pytest

GOL_OK = 0
GOL_EINVAL = -1
GOL_EHIP = -2
GOL_ENOMEM = -3
GOL_EIO = -4
GOL_EFORMAT = -5
GOL_ESTATE = -6
GOL_EQUIT = -7
GOL_ECOMM = -8


def check_program(name):
    """The path of the stand-alone sanitizer program build/asan/`name` (tests/san/`name`.cpp, made by build()); a
    test that asks for one that is not there fails."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gol-distributed-final_amd", "build",
                        "asan", name)
    assert os.path.exists(path), f"build/asan/{name} is missing: run __graft_entry__.build()"
    return path


def _gpu_package():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import golhip
    golhip.lib()
    torch.cuda.set_device(0)
    return golhip


@pytest.fixture(scope="module")
def cpu_lib():
    """The package with its library loaded; no GPU is touched."""
    import golhip
    golhip.lib()
    return golhip


@pytest.fixture(scope="module")
def gpu_lib():
    """The package with its library loaded and device 0 current; skips without a GPU."""
    return _gpu_package()


@pytest.fixture(scope="module")
def env():
    """The raw-ABI tests' namespace: G the package, L the library (GOLHIP_SEQUENCE_LIBRARY names another build to
    run the same cases on), torch, and the status codes they assert."""
    import torch
    G = _gpu_package()
    path = os.environ.get("GOLHIP_SEQUENCE_LIBRARY")
    L = G._lib.load(path) if path else G.lib()
    return types.SimpleNamespace(G=G, L=L, torch=torch, EINVAL=GOL_EINVAL, ESTATE=GOL_ESTATE)


def error_word(G):
    """(rc, flags) of gol_dev_error(-1, ...): the device-side fault word of the current device."""
    flags = ctypes.c_uint32(0xFFFF)
    rc = G.lib().gol_dev_error(-1, ctypes.byref(flags))
    return rc, flags.value


MARGIN = 512  # bytes of `fill` on each side of a Guarded payload (the leading side: MARGIN + off)


class Guarded:
    """`host` (any contiguous array, held as bytes) in a device allocation between two margins of `fill` bytes,
    the payload `off` bytes (0 <= off < 16) past a 16-byte boundary.  .ptr is the payload's address, .before the
    whole allocation as made."""

    def __init__(self, host, fill=0x5A, off=0, device="cuda", name=""):
        import torch
        assert 0 <= off < 16 and MARGIN >= 512 and MARGIN % 16 == 0
        host = np.ascontiguousarray(host)
        self.dtype, self.shape, self.name, self.off = host.dtype, host.shape, name, off
        self.lo, self.nbytes = MARGIN + off, host.nbytes
        self.before = np.full(self.lo + self.nbytes + MARGIN, fill, dtype=np.uint8)
        self.before[self.lo:self.lo + self.nbytes] = host.reshape(-1).view(np.uint8)
        self.t = torch.empty(len(self.before), dtype=torch.uint8, device=device)
        self.t.copy_(torch.from_numpy(self.before))
        assert (self.t.data_ptr() + MARGIN) % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def whole(self):
        """Margins and payload as they are now, as bytes."""
        import torch
        if self.t.is_cuda:
            torch.cuda.synchronize()
        return self.t.cpu().numpy().copy()

    def unchanged(self):
        return np.array_equal(self.whole(), self.before)

    def read(self, dtype=None, shape=None):
        """A copy of the payload (as `dtype`, flat or of `shape`; by default as `host` was) after asserting that both
        margins are byte for byte as made."""
        got, hi = self.whole(), self.lo + self.nbytes
        for side, a, b, at in (("leading", 0, self.lo, -self.lo), ("trailing", hi, len(got), self.nbytes)):
            bad = np.flatnonzero(got[a:b] != self.before[a:b])
            assert bad.size == 0, (f"the {side} margin of {self.name or 'a buffer'} changed: {bad.size} bytes, the first "
                                   f"at payload offset {at + int(bad[0])}")
        if dtype is None:
            dtype, shape = self.dtype, self.shape if shape is None else shape
        out = got[self.lo:hi].copy().view(dtype)
        return out if shape is None else out.reshape(shape)

    def write(self, a):
        """Replaces the payload (on the device; .before stays as made)."""
        import torch
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        assert raw.size == self.nbytes
        self.t[self.lo:self.lo + self.nbytes] = torch.from_numpy(raw.copy()).to(self.t.device)

    def expect(self, want, where=""):
        """The whole allocation, margins included, against `want` as the payload between the margins as made."""
        want = np.ascontiguousarray(want)
        assert want.nbytes == self.nbytes
        w = self.before.copy()
        w[self.lo:self.lo + self.nbytes] = want.reshape(-1).view(np.uint8)
        got = self.whole()
        if np.array_equal(got, w):
            return
        size = want.itemsize
        bad = np.unique((np.flatnonzero(got != w) - self.lo) // size)  # element indices; in a margin: < 0 or >= want.size

        def sample(a):
            at = np.clip(self.lo + bad[:3] * size, 0, len(a) - size)
            return [a[i:i + size].copy().view(want.dtype)[0].tolist() for i in at]

        raise AssertionError(f"{where}: {self.name or 'a buffer'} differs in {bad.size} of {want.size} elements, first at "
                             f"{bad[:6].tolist()} (got {sample(got)}, want {sample(w)})")
