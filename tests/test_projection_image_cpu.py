"""The staged-order weight image of the one-launch projection (csrc/handle.cpp pack_net_image; CPU test: no GPU needed).

mlp_net_kernel's wavefronts copy their weight chunks from memory into their LDS staging buffers by DMA, so memory holds every chunk
as the buffer holds it: [slice of go x b neurons][chunk of ck inputs][go x b staged rows x (ck + 4) floats].  Here the image the
library builds is compared word for word with an independent restatement of what the kernel's register staging used to put into
a buffer, 16-byte piece by piece: piece p of row r of the slice (neuron obase + r, clamped to the layer's last; inputs k0 + 4 p ..
k0 + 4 p + 3, zero from the row's padded end on) goes to staged row (r % b) * go + r / b where the rows are interleaved (go = 4,
b >= 4), r otherwise, float 16 (p / 4) + 2 ((p / 2) % 2) + p % 2 and every fourth float from there.
"""
import ctypes

import numpy as np
import pytest

import gbnns_dim_red_amd as g

NETS = [(128, 256, 32), (200, 72, 32), (96, 128, 64)]
FORMS = {"whole": 2, "half": 4}   # neuron groups per row of 16 lanes


@pytest.fixture(scope="module")
def lib():
    g.build_library()
    lib = g.load_library()
    lib.gbnns_debug_net_image.restype = ctypes.c_int
    lib.gbnns_debug_net_image.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _image(lib, w, din, dout, b, go):
    geom = (ctypes.c_uint64 * 8)()
    b3 = ctypes.c_uint32()
    assert lib.gbnns_debug_net_image(None, w.shape[1], din, dout, b, go, None, 0, geom, ctypes.byref(b3)) == 0
    out = np.full(int(geom[7]), np.float32(np.nan), dtype=np.float32)
    rc = lib.gbnns_debug_net_image(w.ctypes.data, w.shape[1], din, dout, b, go, out.ctypes.data, out.size, geom, None)
    assert rc == 0
    return out, [int(v) for v in geom], int(b3.value)


def _expected(w, din, dout, b, go):
    """What the staging buffers held, piece by piece (the module docstring); padding floats zero."""
    ck = 32 if b >= 4 else 64
    ldw, rows = ck + 4, go * b
    k16 = (din + 15) // 16 * 16
    nch, slices = (din + ck - 1) // ck, (dout + rows - 1) // rows
    interleaved = go == 4 and b >= 4
    img = np.zeros((slices, nch, rows, ldw), dtype=np.float32)
    clamped = zero_tail = 0
    for s in range(slices):
        for c in range(nch):
            for r in range(rows):
                o = s * rows + r
                clamped += o >= dout
                o = min(o, dout - 1)
                sr = (r % b) * go + r // b if interleaved else r
                for p in range(ck // 4):
                    k = c * ck + 4 * p
                    if k < k16:
                        piece = w[o, k:k + 4]
                    else:
                        piece = np.zeros(4, dtype=np.float32)
                        zero_tail += 1
                    at = 16 * (p // 4) + 2 * ((p // 2) % 2) + p % 2
                    img[s, c, sr, at:at + 16:4] = piece
    return img, (ck, ldw, rows, rows * ldw, nch, slices, int(interleaved)), clamped, zero_tail


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("d,dh,dl", NETS, ids=["%d_%d_%d" % n for n in NETS])
def test_image_words_are_the_staged_words(lib, d, dh, dl, form):
    go = FORMS[form]
    rng = np.random.Generator(np.random.PCG64(4200 + d))
    seen = {"clamped": 0, "zero_tail": 0, "pad": 0}
    for l, (din, dout) in enumerate(((d, dh), (dh, dh), (dh, dl))):
        ws = (din + 15) // 16 * 16
        w = np.zeros((dout, ws), dtype=np.float32)
        # every word distinct and non-zero, so that a word in the wrong place cannot pass for the right one
        w[:, :din] = (1 + np.arange(dout * din, dtype=np.float32)).reshape(dout, din) * np.float32(rng.choice([-1.0, 1.0]))
        _, _, b3 = _image(lib, w, din, dout, 8, go)
        assert b3 == (2 if (dout + 15) // 16 <= 2 else 4)
        b = 8 if l < 2 else (2 if (dl + 15) // 16 <= 2 else 4)
        got, geom, _ = _image(lib, w, din, dout, b, go)
        want, wgeom, clamped, zero_tail = _expected(w, din, dout, b, go)
        assert tuple(geom[:7]) == wgeom and geom[7] == want.size, (geom, wgeom)
        got = got.reshape(want.shape)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (l, form, "first differing [slice, chunk, row, float]", bad[0].tolist(), len(bad))
        assert not got[..., geom[0]:].any()                       # the padding floats of every row
        seen["clamped"] += clamped
        seen["zero_tail"] += zero_tail
        seen["pad"] += got[..., geom[0]:].size
        # a chunk is a whole number of 16-byte units and at least one 1-KiB DMA piece, inside the wavefront's staging buffer
        assert geom[3] * 4 % 16 == 0 and geom[3] * 4 >= 1024 and geom[3] <= go * 8 * 36
    assert seen["pad"] > 0
    if (d, dh) == (200, 72):
        assert seen["clamped"] > 0 and seen["zero_tail"] > 0       # 72 neurons in slices of 16 / 32; 208 and 80 padded inputs in chunks of 32


def test_image_refuses_what_is_no_layer(lib):
    geom = (ctypes.c_uint64 * 8)()
    assert lib.gbnns_debug_net_image(None, 128, 128, 256, 3, 2, None, 0, geom, None) != 0
    assert lib.gbnns_debug_net_image(None, 128, 128, 256, 8, 3, None, 0, geom, None) != 0
    assert lib.gbnns_debug_net_image(None, 96, 100, 256, 8, 2, None, 0, geom, None) != 0   # rows shorter than the padded inputs
    w = np.zeros((256, 128), dtype=np.float32)
    out = np.zeros(16, dtype=np.float32)
    assert lib.gbnns_debug_net_image(w.ctypes.data, 128, 128, 256, 8, 2, out.ctypes.data, out.size, geom, None) != 0
