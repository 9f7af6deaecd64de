"""GPU: ingest.decode_jpeg on the designed files of tests/jpeg_dec_cases.py, byte for byte against np.asarray(Image.open(f)), in
mixed batches (designed files, header rewrites and PIL's own files of different sizes in one call) at chunk_bits None, 64, an odd
size and the sizes whose boundary the census puts inside the padding bits; which path took each file is asserted, so that the
PIL fallback cannot hide a failure.  Then a batch of corrupted segments and refused tables next to valid files through
t4d_jpeg_decode itself: the status words of the host build (tests/native/jpeg_host.cpp), PIL's bytes for the neighbours, guard
bytes after the output and the scratch untouched.  tests/test_jpeg_files_host.py holds the census claims of every case and runs
the same inputs through the sanitized host build."""
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageFile

from tests import jpeg_dec_cases as cases
from tests.test_ingest_host import content, jpeg_bytes
from tests.test_jpeg_files_host import ODD, compile_host, descriptor, host_run
from topo4d_amd import _lib, ingest
from topo4d_amd._lib import ptr

pytestmark = pytest.mark.gpu
ImageFile.MAXBLOCK = 1 << 24


def pil(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def pil_files():
    """PIL's own files of different sizes, samplings and table kinds, to sit between the designed ones."""
    return [jpeg_bytes(content(h, w, kind, seed=i), quality=q, subsampling=sub, **kw)
            for i, ((h, w), kind, q, sub, kw) in enumerate([((17, 33), "noise", 90, 2, {}), ((72, 96), "grad", 75, 1, {"optimize": True}),
                                                            ((1, 1), "flat", 50, 0, {}), ((40, 56), "saturated", 100, 0, {"restart_marker_blocks": 3}),
                                                            ((64, 64), "noise", 95, 2, {"restart_marker_rows": 1})])]


def mixed(files):
    """`files` with one of PIL's own after every seventh."""
    extra, out = pil_files(), []
    for k, f in enumerate(files):
        out.append(f)
        if k % 7 == 6:
            out.append(extra[(k // 7) % len(extra)])
    return out


def decode_and_check(files, chunk_bits, taken=True):
    """Every file through decode_jpeg in one call; each equals PIL, and each took the path `taken` says (True: the GPU decoder)."""
    for k, f in enumerate(files):
        assert ingest.parse_jpeg(f).gpu == taken, (k, ingest.parse_jpeg(f).reason)
    out = ingest.decode_jpeg(files, chunk_bits=chunk_bits)
    assert len(out) == len(files)
    bad = []
    for k, (f, o) in enumerate(zip(files, out)):
        want = pil(f)
        got = o.cpu().numpy()
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((k, chunk_bits, want.shape))
    return bad


@pytest.fixture(scope="module")
def designed():
    taken, _ = cases.header_cases()
    files = [c.data for c in cases.all_cases()] + [data for _, data, _ in taken]
    names = [c.name for c in cases.all_cases()] + [name for name, _, _ in taken]
    return names, files


@pytest.mark.parametrize("chunk_bits", [None, 64, ODD])
def test_designed_files_in_mixed_batches(designed, chunk_bits):
    names, files = designed
    batch = mixed(files)
    bad = decode_and_check(batch, chunk_bits)
    index = {id(f): n for n, f in zip(names, files)}
    assert not bad, [(index.get(id(batch[k]), "pil"), cb) for k, cb, _ in bad[:10]]


def test_headers_the_gpu_path_does_not_take(designed):
    _, not_taken = cases.header_cases()
    for name, data, base, reason in not_taken:
        h = ingest.parse_jpeg(data)
        assert not h.gpu and h.reason == reason, (name, h.reason)
    files = [data for _, data, _, _ in not_taken]
    assert not decode_and_check(files, None, taken=False)
    both = [f for pair in zip(files, designed[1]) for f in pair]         # and interleaved with files the GPU takes
    out = ingest.decode_jpeg(both, chunk_bits=ODD)
    assert all(np.array_equal(o.cpu().numpy(), pil(f)) for f, o in zip(both, out))


def test_chunk_boundary_inside_padding():
    """data_bits + 1, its divisors >= 64 and 65, 67, 101, 127, 250 on files whose census puts a boundary of such a chunk strictly
    inside the padding bits (asserted here again for the sizes the test relies on)."""
    chunk = cases.chunk_cases()
    files = [c.data for c, _, _ in chunk]
    covered = set()
    for c, sizes, hit in chunk:
        for cb in hit:
            m = (c.census["data_bits"] + c.census["pad_bits"] - 1) // cb
            assert c.census["data_bits"] < m * cb < c.census["data_bits"] + c.census["pad_bits"]
        covered |= set(hit)
    assert covered >= set(cases.FIXED_CHUNKS)
    bad = []
    for cb in sorted({cb for _, sizes, _ in chunk for cb in sizes}):
        bad += decode_and_check(files, cb)
    assert not bad, bad[:10]


def test_rejected_chunk_sizes_raise_before_any_launch():
    f = [cases.base_files()[0].data]
    for cb in (1, 8, 63, -64):
        with pytest.raises(ValueError, match="chunk_bits"):
            ingest.decode_jpeg(f, chunk_bits=cb)


def test_with_and_without_the_sequential_fallback():
    """The cases the host build must finish with the fallback, and those it must finish without (test_jpeg_files_host.py asserts
    its exit status exactly), against PIL."""
    by = {}
    for c, cb, fallback in cases.fallback_cases():
        by.setdefault(cb, []).append(c.data)
    assert any(fb for _, _, fb in cases.fallback_cases()) and not all(fb for _, _, fb in cases.fallback_cases())
    bad = []
    for cb, files in sorted(by.items()):
        bad += decode_and_check(files + pil_files()[:2], cb or None)
    assert not bad, bad


def test_odd_byte_offset_in_the_packed_buffer(designed):
    names, files = designed
    odd = [f for f in files if (ingest.parse_jpeg(f).scan_end - ingest.parse_jpeg(f).scan_start) % 2 == 1]
    assert odd
    batch = [odd[0]] + mixed(files[:40])
    assert not decode_and_check(batch, None) and not decode_and_check(batch, ODD)


def test_scratch_prefilled(designed, monkeypatch):
    """Nothing reads scratch it has not written: the same results over scratch filled with 0xAB."""
    real = _lib.scratch
    seen = []

    def filled(query, device, *args, **kw):
        t, n = real(query, device, *args, **kw)
        t.fill_(0xAB)
        seen.append(query)
        return t, n
    monkeypatch.setattr(_lib, "scratch", filled)
    names, files = designed
    batch = mixed(files[::3]) + [c.data for c, _, _ in cases.chunk_cases()]
    assert not decode_and_check(batch, ODD) and not decode_and_check(batch, None)
    assert seen == ["t4d_jpeg_scratch_bytes"] * 2


GUARD = 4096


def test_corrupted_and_refused_inputs_next_to_valid_files(tmp_path):
    """About a dozen of the corrupted inputs the sanitized host build runs clean (test_jpeg_files_host.py), refused tables
    among them, alternating with valid files in one t4d_jpeg_decode call: the host build's status bits, PIL's bytes for the valid
    files (and the host build's bytes for a corrupted segment that still decodes), guards untouched."""
    exe = compile_host(tmp_path / "jpeg_host", ["-O2"])
    corrupt = cases.corrupted()
    refused = [c for c in corrupt if c.tables]
    others = [c for c in corrupt if not c.tables]
    chosen = others[::max(1, len(others) // 9)][:9] + [refused[0], refused[5], refused[-1]]
    assert len({c.name.split("-")[-1].rstrip("0123456789") for c in chosen}) >= 6
    valid = [c.data for c in cases.base_files()] + pil_files()
    dev = torch.device("cuda", torch.cuda.current_device())
    items = []                                                      # (header, segment, tables, expected pixels or None, status)
    for k, c in enumerate(chosen):
        f = valid[k % len(valid)]
        h = ingest.parse_jpeg(f)
        items.append((h, f[h.scan_start:h.scan_end], None, pil(f).tobytes(), 0))
        rc, out = host_run(exe, descriptor(c.header, len(c.segment), c.tables), ODD, c.segment)
        items.append((c.header, c.segment, c.tables, out if rc in (0, 128) else None, 0 if rc == 128 else rc))
    assert sum(1 for it in items if it[4]) >= 8 and any(it[4] & 4 for it in items if it[2])
    descs = (_lib.T4DJpegImage * len(items))()
    data_off = out_off = 0
    for k, (h, seg, tables, _, _) in enumerate(items):
        descs[k] = descriptor(h, len(seg), tables, data_off, out_off)
        data_off += len(seg)
        out_off += h.width * h.height * 3
    data = torch.frombuffer(bytearray(b"".join(it[1] for it in items)), dtype=torch.uint8).to(dev)
    d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    nscratch = int(_lib.load().t4d_jpeg_scratch_bytes(descs, len(items), ODD))
    assert nscratch > 0
    scratch = torch.full((nscratch + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    pixels = torch.full((out_off + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    status = torch.full((len(items) + 16,), -7, dtype=torch.int32, device=dev)
    _lib.call("t4d_jpeg_decode", descs, ptr(d_descs), len(items), ptr(data), ODD, ptr(pixels), out_off, ptr(status), ptr(scratch),
              nscratch, _lib.stream(dev))
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    px = pixels.cpu().numpy()
    assert st[len(items):] == [-7] * 16
    assert (px[out_off:] == 0xCD).all() and bool((scratch[nscratch:] == 0xAB).all())
    assert st[:len(items)] == [it[4] for it in items], list(zip(st, [it[4] for it in items]))
    for k, (h, _, _, want, _) in enumerate(items):
        if want is not None:
            o = descs[k].out_offset
            assert px[o:o + len(want)].tobytes() == want, k
