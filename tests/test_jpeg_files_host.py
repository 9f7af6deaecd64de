"""CPU: the designed JPEG files of tests/jpeg_dec_cases.py - their census claims, the header parser's verdict on every rewrite, and
the host build of csrc/t4d_jpeg.h (tests/native/jpeg_host.cpp) against PIL, byte for byte: at chunk sizes whose boundary falls
inside the padding bits, with and without the sequential fallback (exact exit status), and, built with
-fsanitize=address,undefined, over every designed case and a seeded set of corrupted segments and refused tables."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageFile

from tests import jpeg_dec_cases as cases
from tests import jpeg_files as jf
from tests.test_ingest_host import content, jpeg_bytes
from topo4d_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "jpeg_host.cpp")
ImageFile.MAXBLOCK = 1 << 24
OPS = {"eq": lambda a, b: a == b, "ge": lambda a, b: a >= b, "le": lambda a, b: a <= b}
ODD = 67                                # the odd chunk size of the runs over all cases


def compile_host(path, flags):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(path), SRC])
    return str(path)


@pytest.fixture(scope="module")
def jpeg_host(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("native") / "jpeg_host", ["-O2"])


@pytest.fixture(scope="module")
def jpeg_host_san(tmp_path_factory):
    return compile_host(tmp_path_factory.mktemp("native") / "jpeg_host_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def pil(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def descriptor(header, segment_bytes, tables=None, data_offset=0, out_offset=0):
    """ingest's descriptor of a parsed file, for a segment of `segment_bytes` bytes, with {slot: bits[16]} written over its
    Huffman tables' counts."""
    d = ingest._descriptor(header, data_offset, out_offset)
    d.data_bytes = segment_bytes
    for slot, bits in (tables or {}).items():
        C.memmove(C.addressof(d.huff_bits[slot]), bytes(bits), 16)
    return d


def host_run(exe, desc, chunk_bits, segment):
    """(exit status, stdout) of the host build; a sanitizer report, which goes to stderr, fails here."""
    r = subprocess.run([exe], input=bytes(desc) + struct.pack("<i", chunk_bits) + bytes(segment), capture_output=True)
    assert r.stderr == b"" and 0 <= r.returncode <= 128, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.returncode, r.stdout


def host_file(exe, data, chunk_bits):
    h = ingest.parse_jpeg(data)
    assert h.gpu, h.reason
    seg = data[h.scan_start:h.scan_end]
    return host_run(exe, descriptor(h, len(seg)), chunk_bits, seg)


# ---- the census ----------------------------------------------------------------------------------------------------------------
def test_claims():
    every = cases.all_cases() + [c for c, _, _ in cases.chunk_cases()] + [c for c, _, _ in cases.fallback_cases()]
    names = [c.name for c in cases.all_cases()]
    assert len(set(names)) == len(names)
    for c in every + [cases.beyond_range()]:
        assert ingest.parse_jpeg(c.data).width <= 96 and ingest.parse_jpeg(c.data).height <= 72
        for key, (op, value) in c.claims.items():
            assert OPS[op](c.census[key], value), (c.name, key, op, value, c.census[key])
    for c in every:                                          # the range condition, whatever else a case claims
        assert -cases.RANGE <= c.census["sample_min"] and c.census["sample_max"] <= cases.RANGE, c.name
        assert c.census["max_dequant"] < 32768, c.name


def test_block_cases_cover_what_the_issue_lists():
    """Per sampling: every position with both signs at magnitude 1 and at the largest magnitude, DC category 11, AC category 10,
    one to three ZRLs, a term on index 63, EOB-only and full blocks, all under four tables."""
    by = {}
    for c in cases.block_cases():
        by.setdefault(c.name.split("[")[0], []).append(c)
    assert len(by) == 7 * 3 * 4
    for s in ("1x1", "2x1", "2x2"):
        assert max(c.census["max_dc_category"] for c in by[f"dc_swing-{s}-ones"]) == 11
        assert max(c.census["max_ac_category"] for c in by[f"ac_cat10-{s}-ones"]) == 10
        for qn, (ql, qc) in cases.QUANTS.items():
            assert sum(c.census["blocks"] for c in by[f"single-{s}-{qn}"]) >= 256
            assert all(c.census["max_zrl_run"] == 3 for c in by[f"zrl-{s}-{qn}"])
    h = ingest.parse_jpeg(by["single-1x1-all255"][0].data)
    assert h.gpu and all((q == 255).all() for q in h.quant.values())


def test_padding_cases_cover_every_length_and_both_bits():
    got = {(c.census["pad_bits"], c.name.endswith("bit1")) for c in cases.padding_cases()}
    assert got == {(p, b) for p in range(8) for b in (False, True)}
    for c in cases.padding_cases():
        h = ingest.parse_jpeg(c.data)
        end = h.scan_end - 1 if c.data[h.scan_end - 2:h.scan_end] == b"\xff\x00" else h.scan_end      # a stuffed last byte
        last = c.data[end - 1]
        n = c.census["pad_bits"]
        assert last & ((1 << n) - 1) == ((1 << n) - 1 if c.name.endswith("bit1") else 0)


def test_table_cases_use_the_tables_they_name():
    for c in cases.table_cases():
        h = ingest.parse_jpeg(c.data)
        assert h.gpu, (c.name, h.reason)
        if c.name.startswith("four_tables"):
            assert len(h.huffman) == 8 and len({(tuple(b), bytes(v)) for b, v in h.huffman.values()}) == 8
            assert h.scan[1][1:] != h.scan[2][1:] and h.scan[0][1:] != h.scan[1][1:]
        if c.name.startswith("three_quant"):
            assert [t for _, _, _, t in h.components] == [0, 1, 2] and len({q.tobytes() for q in h.quant.values()}) == 3
        if c.name.startswith("dqt16"):
            assert max(int(q.max()) for q in h.quant.values()) > 255
        if c.name.startswith("writer_layout"):
            assert h.sof == 1 and not h.jfif and h.restart_interval == 3 and [x[0] for x in h.components] == [7, 200, 0]
            assert sorted(h.quant) == [2, 3] and sorted(h.huffman) == [(0, 2), (0, 3), (1, 2), (1, 3)]
            head = c.data[:h.scan_start]
            assert head.count(b"\xff\xc4") == 1 and head.index(b"\xff\xc4") < head.index(b"\xff\xc1") < head.index(b"\xff\xdb")
        if c.name.startswith("one_symbol_ac"):
            assert sum(h.huffman[(1, 0)][0]) == 1


# ---- the host build against PIL --------------------------------------------------------------------------------------------------
def test_host_build_matches_pil_on_designed_cases(jpeg_host):
    bad = []
    for c in cases.all_cases():
        want = pil(c.data).tobytes()
        for cb in (0, 64, ODD):
            rc, out = host_file(jpeg_host, c.data, cb)
            if out != want or rc not in ((0,) if cb == 0 or "rst" in c.name else (0, 128)):
                bad.append((c.name, cb, rc))
    assert not bad, bad[:10]


def test_header_rewrites_are_taken_and_decode_as_their_base(jpeg_host):
    taken, not_taken = cases.header_cases()
    assert len(taken) == 14 * 6 and len(not_taken) == 3 * 6
    for name, data, base in taken:
        h = ingest.parse_jpeg(data)
        assert h.gpu, (name, h.reason)
        want = pil(base.data)
        assert np.array_equal(pil(data), want), name
        for cb in (0, ODD):
            rc, out = host_file(jpeg_host, data, cb)
            assert out == want.tobytes(), (name, cb, rc)
    for name, data, base, reason in not_taken:
        h = ingest.parse_jpeg(data)
        assert not h.gpu and h.reason == reason, (name, h.reason)
        assert pil(data).shape == pil(base.data).shape, name


def test_rewrites_change_what_they_name():
    b = cases.base_files()[0]
    h0 = ingest.parse_jpeg(b.data)
    h = {name: ingest.parse_jpeg(f(b.data)) for name, f in jf.REWRITES.items()}
    assert h["renumbered_sof1"].sof == 1 and [c[0] for c in h["renumbered_sof1"].components] == [7, 200, 0]
    assert sorted(h["renumbered_sof1"].quant) == [2, 3] and sorted(h["renumbered_sof1"].huffman) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    assert h["renumbered_sof1"].jfif and not h["renumbered_sof1_no_jfif"].jfif
    assert h["separate_cr_tables"].scan[2][1:] == (2, 2) and h["separate_cr_tables"].components[2][3] == 2
    assert h["adobe_1_no_jfif"].adobe_transform == 1 and not h["adobe_1_no_jfif"].jfif and h["adobe_1_jfif"].jfif
    assert h["dri_0"].restart_interval == 0 and h["dri_65535"].restart_interval == 65535
    assert b"\x10" + b"\x00" in jf.dqt_16bit(b.data)[:200] and jf.dqt_16bit(b.data).count(b"\xff\xdb") >= 2
    assert jf.tables_merged(b.data).count(b"\xff\xc4\x01\xa2") == 1
    assert b"\xff\xd9\xff\xda" in jf.exif_and_com(b.data)[:h["exif_and_com"].scan_start]
    assert jf.exif_and_com(b.data)[:h["exif_and_com"].scan_start].count(b"\xff\xd8") == 2
    assert jf.ff_fill(b.data)[2:6] == b"\xff\xff\xff\xff"
    after = jf.bytes_after_eoi(b.data)
    assert after.startswith(b.data) and len(after) > len(b.data) and h["bytes_after_eoi"].scan_end == h0.scan_end
    assert h["dqt_16bit"].quant.keys() == h0.quant.keys() and all(np.array_equal(h["dqt_16bit"].quant[t], q) for t, q in h0.quant.items())
    r = cases.base_files()[2]
    assert ingest.parse_jpeg(jf.REWRITES["dri_0"](r.data)).restart_interval == 2


def test_beyond_the_range_condition_the_decoder_and_pil_differ(jpeg_host):
    """The rule of t4d_jpeg.h's range_limit comment: past an exact sample of +-512 libjpeg's C range table wraps (what the decoder
    restates) and PIL's SIMD IDCT saturates.  If this stops failing to match, the rule in DESIGN.md has changed."""
    c = cases.beyond_range()
    assert c.census["sample_max"] >= 512 and c.census["sample_min"] <= -513
    rc, out = host_file(jpeg_host, c.data, 0)
    want = pil(c.data)
    got = np.frombuffer(out, np.uint8).reshape(want.shape)
    assert rc == 0 and (got != want).any()
    flat = want.shape[0] * want.shape[1]
    assert (got != want).any(-1).sum() < flat              # and only some samples differ: the blocks inside the range agree


# ---- chunk sizes -----------------------------------------------------------------------------------------------------------------
def test_chunk_boundary_inside_padding(jpeg_host):
    """Every accepted chunk_bits decodes every valid file: data_bits + 1, its divisors >= 64 and the sizes 65, 67, 101, 127, 250,
    on files whose census proves that a chunk boundary falls strictly inside the padding bits."""
    covered = set()
    for c, sizes, hit in cases.chunk_cases():
        assert hit and c.census["pad_bits"] >= 2 and c.census["data_bits"] + 1 in hit
        for cb in hit:
            m = (c.census["data_bits"] + c.census["pad_bits"] - 1) // cb
            assert c.census["data_bits"] < m * cb < c.census["data_bits"] + c.census["pad_bits"] and cb >= 64
        covered |= set(hit)
        want = pil(c.data).tobytes()
        for cb in sizes:
            rc, out = host_file(jpeg_host, c.data, cb)
            assert rc in (0, 128) and out == want, (c.name, cb, rc)
    assert covered >= set(cases.FIXED_CHUNKS)


def test_pil_files_decode_at_every_chunk_size(jpeg_host):
    """PIL's own files (four sizes, three samplings, three qualities, four contents) at byte-multiple and other chunk sizes."""
    bad = []
    i = 0
    for (h, w) in [(17, 33), (40, 56), (64, 64), (72, 96)]:
        for sub in (0, 1, 2):
            for q in (50, 90, 100):
                for kind in ("noise", "flat", "saturated", "grad"):
                    i += 1
                    data = jpeg_bytes(content(h, w, kind, seed=i), quality=q, subsampling=sub)
                    want = pil(data).tobytes()
                    for cb in (64, 65, 67, 100, 101, 127, 250, 1001):
                        rc, out = host_file(jpeg_host, data, cb)
                        if rc not in (0, 128) or out != want:
                            bad.append((h, w, sub, q, kind, cb, rc))
    assert not bad, (len(bad), bad[:10])


# ---- the sequential fallback -----------------------------------------------------------------------------------------------------
def test_fallback_runs_exactly_where_named(jpeg_host):
    for c, cb, fallback in cases.fallback_cases():
        rc, out = host_file(jpeg_host, c.data, cb)
        assert rc == (128 if fallback else 0), (c.name, cb, rc)
        assert out == pil(c.data).tobytes(), (c.name, cb)


# ---- the sanitized build ---------------------------------------------------------------------------------------------------------
def test_sanitized_build_on_designed_cases(jpeg_host_san):
    every = cases.all_cases() + [c for c, _, _ in cases.chunk_cases()]
    for c in every:
        want = pil(c.data).tobytes()
        for cb in (0, 64, ODD):
            rc, out = host_file(jpeg_host_san, c.data, cb)
            assert rc in (0, 128) and out == want, (c.name, cb, rc)


def test_sanitized_build_on_corrupted_input(jpeg_host_san, jpeg_host):
    """No sanitizer report (host_run asserts an empty stderr) on corrupted segments and refused tables; a refused table reports
    bit 4; the plain build agrees on the status."""
    corrupt = cases.corrupted()
    kinds = {c.name.split("-")[-1].rstrip("0123456789") for c in corrupt}
    assert kinds >= {"flip", "random", "ff_run", "zero_run", "junk", "cut", "rst_dropped", "rst_doubled", "rst_swapped",
                     "rst_all_dropped", "refused_overfull", "refused_all_ones", "refused_too_many", "refused_all_tables"}
    rejected = 0
    for c in corrupt:
        d = descriptor(c.header, len(c.segment), c.tables)
        for cb in (0, 64, ODD):
            rc, out = host_run(jpeg_host_san, d, cb, c.segment)
            rejected += rc not in (0, 128)
            if c.tables:
                assert rc & 4 and rc < 128, (c.name, cb, rc)
            if rc in (0, 128):
                assert len(out) == c.header.width * c.header.height * 3
            if cb == ODD:
                assert host_run(jpeg_host, d, cb, c.segment) == (rc, out), c.name
    assert rejected > len(corrupt)                          # most corruptions are noticed


def test_uncorrupted_segments_through_the_same_path(jpeg_host_san):
    for c in cases.base_files():
        h = ingest.parse_jpeg(c.data)
        seg = c.data[h.scan_start:h.scan_end]
        rc, out = host_run(jpeg_host_san, descriptor(h, len(seg)), ODD, seg)
        assert rc in (0, 128) and out == pil(c.data).tobytes()
