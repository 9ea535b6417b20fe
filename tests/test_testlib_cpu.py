"""The net under the kernel tests, tested: tests/testlib.py's Guarded on a CPU tensor (the same code path as on
the device) sees a byte written on either side of its payload, at the payload's edge and at the margin's far end;
the status codes it pins are golhip._lib's and include/golhip.h's; and no file of tests/ imports a test module."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import island_ref as I
import testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
PAYLOADS = {"uint8-1": np.array([7], dtype=np.uint8), "int64-37": np.arange(-5, 32, dtype=np.int64),
            "records-13": np.arange(13 * 24, dtype=np.uint8).view(I.DTYPE)}
assert I.DTYPE.itemsize == 24


def _poke(address, xor=0xFF):
    byte = ctypes.c_uint8.from_address(address)
    byte.value ^= xor


@pytest.fixture(params=[(k, off) for k in PAYLOADS for off in (0, 5)], ids=lambda p: f"{p[0]}-off{p[1]}")
def made(request):
    key, off = request.param
    host = PAYLOADS[key]
    return host, off, T.Guarded(host, fill=0xA5, off=off, device="cpu", name="probe")


def test_untouched(made):
    host, off, g = made
    assert T.MARGIN >= 512 and T.MARGIN % 16 == 0 and (g.ptr - off) % 16 == 0
    assert g.ptr - g.t.data_ptr() == T.MARGIN + off and len(g.before) == 2 * T.MARGIN + off + host.nbytes
    assert set(g.before[:T.MARGIN + off].tolist()) == set(g.before[-T.MARGIN:].tolist()) == {0xA5}
    assert g.unchanged() and np.array_equal(g.whole(), g.before)
    got = g.read()
    assert got.dtype == host.dtype and got.shape == host.shape and got.tobytes() == host.tobytes()
    assert g.read(np.uint8).tobytes() == host.tobytes() and g.read(np.uint8, (1, -1)).shape == (1, host.nbytes)
    g.expect(host)
    got[...] = got[::-1]  # a copy: the buffer stays
    assert g.unchanged()


@pytest.mark.parametrize("place", ["ptr - 1", "ptr + nbytes", "first of leading", "last of trailing"])
def test_a_byte_outside_the_payload(made, place):
    host, off, g = made
    at = {"ptr - 1": -1, "ptr + nbytes": host.nbytes, "first of leading": -(T.MARGIN + off),
          "last of trailing": host.nbytes + T.MARGIN - 1}[place]
    side = "leading" if at < 0 else "trailing"
    _poke(g.ptr + at)
    with pytest.raises(AssertionError, match=rf"the {side} margin of probe changed: 1 bytes, the first at payload offset {at}\b"):
        g.read()
    assert not g.unchanged()
    with pytest.raises(AssertionError, match="probe differs in 1 of"):
        g.expect(host, "here")
    _poke(g.ptr + at)
    assert g.unchanged() and g.read().tobytes() == host.tobytes()


def test_a_byte_inside_the_payload(made):
    host, off, g = made
    k = host.size - 1  # the last element, its second byte if it has one
    at = k * host.itemsize + min(1, host.itemsize - 1)
    _poke(g.ptr + at, 0x10)
    want = host.copy().reshape(-1).view(np.uint8)
    want[at] ^= 0x10
    assert g.read().tobytes() == want.tobytes() and not g.unchanged()
    with pytest.raises(AssertionError, match=rf"here: probe differs in 1 of {host.size} elements, first at \[{k}\] "):
        g.expect(host, "here")
    g.expect(want.view(host.dtype))


def test_write_then_read(made):
    host, off, g = made
    new = (host.copy().reshape(-1).view(np.uint8) ^ 0x3C).view(host.dtype)
    g.write(new)
    assert g.read().tobytes() == new.tobytes() and not g.unchanged()
    g.expect(new)
    whole = g.whole()
    assert np.array_equal(whole[:T.MARGIN + off], g.before[:T.MARGIN + off]) and np.array_equal(whole[-T.MARGIN:], g.before[-T.MARGIN:])
    with pytest.raises(AssertionError):
        g.write(np.zeros(host.nbytes + 1, dtype=np.uint8))


def test_status_codes_are_the_librarys_and_the_headers():
    from golhip import _lib
    names = ["GOL_OK", "GOL_EINVAL", "GOL_EHIP", "GOL_ENOMEM", "GOL_EIO", "GOL_EFORMAT", "GOL_ESTATE", "GOL_EQUIT", "GOL_ECOMM"]
    mine = {k: getattr(T, k) for k in names}
    assert mine == {k: v for k, v in vars(T).items() if re.fullmatch(r"GOL_(OK|E[A-Z]+)", k)}
    assert list(mine.values()) == [0, -1, -2, -3, -4, -5, -6, -7, -8]
    assert mine == {k: getattr(_lib, k) for k in names}
    with open(os.path.join(HERE, "..", "include", "golhip.h")) as f:
        header = f.read()
    # (the header states them as the enumerators of one enum or as #define lines)
    found = re.findall(r"^\s*(?:#define\s+)?(GOL_(?:OK|E[A-Z]+))\s*=?\s*\(?(-?\d+)\)?\s*,?\s*(?:/\*.*)?$", header, re.M)
    assert {k: int(v) for k, v in found} == mine


def test_no_file_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(HERE, "*.py")))
    assert len(files) > 60
    for path in files:
        with open(path) as f:
            bad = [line for line in f if re.match(r"\s*(from|import) test_", line)]
        assert not bad, (os.path.basename(path), bad)
