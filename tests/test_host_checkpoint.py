"""Checkpoint blobs (include/chem_mi355.h, chem_checkpoint_save / chem_checkpoint_load), host side: the writer, the reader, the
fingerprint compare and the checksum of chemlab_amd/csrc/chem_ckpt_host.hpp through tests/host/checkpoint_harness.cpp.  Round
trips of synthetic states (every section filled; empty lists, no fix sets, no events), save -> load -> save byte for byte, and
every refusal by name: a blob cut at every section boundary and one byte short, a flipped magic, version, precision or checksum,
a section length beyond the rest, counts that overflow, a fingerprint that differs in each single field.  The blobs are taken
apart here by the layout the header documents, so the format is pinned as well.  Nothing here needs a GPU.  The harness is
compiled with g++ from tests/host/, once more with -fsanitize=address,undefined as a stand-alone program: it reads every blob
from a heap block of exactly its size, so a read past nbytes is a report."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAGIC, END = 0x4B434843, 0x21444E45
SECTIONS = ["fingerprint", "core", "barostat", "particles", "resolution", "lists", "exclusions", "graph", "fix", "removed", "events", "atrp", "end"]
# (npart, reactions, dissociations, fix sets, atrp, lists as (arity, kind, by_types, hybrid))
FULL = (12, 2, 1, 2, 1, [(2, 1, 0, 1), (3, 10, 0, 0), (4, 20, 1, 0), (2, 5, 1, 0)])
BARE = (5, 0, 0, 0, 0, [])


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "checkpoint_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "checkpoint_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "checkpoint_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    return [x for x in out.stdout.split("\n") if x]


def fp_line(fp):
    n, nr, nd, nf, atrp, lists = fp
    return "fp %d %d %d %d %d %d %s" % (n, nr, nd, nf, atrp, len(lists), " ".join("%d %d %d %d" % l for l in lists))


def fnv(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def walk(blob):
    """[(name, offset of the section header, offset of the payload, length)] by the documented layout"""
    out, pos = [], 16
    for name in SECTIONS:
        sid, zero, ln = struct.unpack_from("<IIQ", blob, pos)
        assert zero == 0 and sid == (END if name == "end" else SECTIONS.index(name) + 1), (name, sid)
        out.append((name, pos, pos + 16, ln))
        pos += 16 + ln
    assert pos == len(blob)
    return out


def resum(blob):
    """the blob with its checksum made right again (what a corruption that is not caught by the sum looks like)"""
    b = bytearray(blob)
    struct.pack_into("<Q", b, len(b) - 8, fnv(bytes(b[:len(b) - 8])))
    return bytes(b)


def make_blob(exe, fp, seed, mode, prec=64):
    out = drive(exe, [fp_line(fp), "prec %d" % prec, "synth %d %s" % (seed, mode), "sizes", "write", "hex"])
    sizes = [int(v) for v in out[0].split()[1:]]
    blob = bytes.fromhex(out[2].split()[1])
    assert out[1] == "wrote %d" % len(blob)
    return blob, sizes


def read_blob(exe, fp, blob, prec=64, seed=None, mode="full", extra=()):
    """the harness's answer to reading `blob` under fingerprint fp (+ extra fpset lines); with a seed the state it held before
    is the synthetic one, and "same" says whether it still is afterwards"""
    lines = [fp_line(fp), "prec %d" % prec]
    if seed is not None:
        lines.append("synth %d %s" % (seed, mode))
    lines += list(extra) + ["blob " + blob.hex(), "read"] + (["same"] if seed is not None else [])
    return drive(exe, lines)


def refused(out, *words):
    assert out[0].startswith("read %d checkpoint: " % EINVAL), out
    for w in words:
        assert w in out[0], (w, out[0])
    return out[0]


@pytest.mark.parametrize("prec", [64, 32])
def test_round_trip_with_every_section_filled(harness, prec):
    blob, sizes = make_blob(harness, FULL, 11, "full", prec)
    assert all(s > 0 for s in sizes), sizes                      # particles, stamps, entries, births, exclusions, graph, fix entries, both logs, removed, events, blocks, atrp
    secs = walk(blob)
    assert struct.unpack_from("<IIII", blob, 0) == (MAGIC, 1, prec, 0)
    assert all(ln > 0 for _, _, _, ln in secs) and secs[-1][3] == 8
    assert struct.unpack_from("<Q", blob, len(blob) - 8)[0] == fnv(blob[:-8])
    out = drive(harness, [fp_line(FULL), "prec %d" % prec, "synth 11 full", "write", "synth 99 empty", "blob " + blob.hex(), "read", "sizes", "write", "hex",
                          "synth 11 full", "blob " + blob.hex(), "read", "same"])
    assert out[1] == "read 0" and [int(v) for v in out[2].split()[1:]] == sizes
    assert bytes.fromhex(out[4].split()[1]) == blob                                 # save -> load -> save: the same bytes
    assert out[5] == "read 0" and out[6] == "same 1"                                # and the same state, field by field


@pytest.mark.parametrize("fp", [FULL, BARE], ids=["lists_and_sets", "bare"])
def test_round_trip_of_an_empty_state(harness, fp):
    """Empty lists, no live fix entry (or no fix set at all), an event log of 0 records, no stamps, no ATRP row."""
    blob, sizes = make_blob(harness, fp, 3, "empty")
    assert sizes[0] == fp[0] and not any(sizes[1:]), sizes
    out = drive(harness, [fp_line(fp), "synth 3 empty", "blob " + blob.hex(), "read", "same", "write", "hex"])
    assert out[0] == "read 0" and out[1] == "same 1"
    assert bytes.fromhex(out[3].split()[1]) == blob


def test_cut_blobs_are_refused_and_nothing_changes(harness):
    blob, _ = make_blob(harness, FULL, 5, "full")
    cuts = {0, 8, 15, 16, len(blob) - 1, len(blob) - 8, len(blob) - 9}
    for name, hdr, payload, ln in walk(blob):
        cuts.update((hdr, hdr + 8, payload, payload + ln // 2))
    assert len(cuts) > 3 * len(SECTIONS)
    for cut in sorted(cuts):
        out = read_blob(harness, FULL, blob[:cut], seed=5)
        refused(out, "truncated")
        assert out[1] == "same 1", cut


def test_flipped_header_words_and_checksum_are_named(harness):
    blob, _ = make_blob(harness, FULL, 6, "full")

    def patched(off, fmt, v):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)
    refused(read_blob(harness, FULL, patched(0, "<I", MAGIC ^ 1)), "bad magic")
    refused(read_blob(harness, FULL, patched(4, "<I", 2)), "unknown format version 2")
    refused(read_blob(harness, FULL, patched(8, "<I", 32)), "precision mismatch", "CHEM_PREC_F32", "CHEM_PREC_F64")
    refused(read_blob(harness, FULL, blob, prec=32), "precision mismatch")                  # an fp64 blob into an fp32 context
    refused(read_blob(harness, FULL, patched(len(blob) - 8, "<Q", fnv(blob[:-8]) ^ 1)), "checksum mismatch")
    for off in (40, len(blob) // 2, len(blob) - 30):                                          # any flipped payload bit
        b = bytearray(blob)
        b[off] ^= 0x10
        out = read_blob(harness, FULL, bytes(b), seed=6)
        refused(out)
        assert out[1] == "same 1"
    refused(read_blob(harness, FULL, blob + b"\0"), "1 bytes behind the last section")
    refused(read_blob(harness, FULL, b""), "truncated")


def test_lengths_and_counts_that_overflow(harness):
    blob, _ = make_blob(harness, FULL, 7, "full")
    secs = {name: (hdr, payload, ln) for name, hdr, payload, ln in walk(blob)}
    for name in SECTIONS[:-1]:                                   # a section length larger than the rest of the blob
        b = bytearray(blob)
        struct.pack_into("<Q", b, secs[name][0] + 8, len(blob))
        refused(read_blob(harness, FULL, resum(bytes(b))), "section " + name, "larger than the rest")
        struct.pack_into("<Q", b, secs[name][0] + 8, 2 ** 64 - 8)
        refused(read_blob(harness, FULL, resum(bytes(b))), "section " + name, "larger than the rest")
    # a section one word shorter, the next one moved up: the walk no longer finds the next header
    b = bytearray(blob)
    struct.pack_into("<Q", b, secs["core"][0] + 8, secs["core"][2] - 8)
    refused(read_blob(harness, FULL, resum(bytes(b))), "corrupt", "section barostat expected")
    # counts: the first word of these sections' payloads is an array count (or a record count)
    for name, each in (("particles", 8), ("resolution", 8), ("lists", 16), ("exclusions", 4), ("graph", 4), ("fix", 16), ("removed", 24), ("events", 4)):
        for count in (2 ** 61 + 1, 2 ** 64 - 1, secs[name][2] // each + 1):
            b = bytearray(blob)
            struct.pack_into("<Q", b, secs[name][1], count)
            out = read_blob(harness, FULL, resum(bytes(b)), seed=7)
            refused(out, "section " + name, "overflows the section")
            assert out[1] == "same 1"
    # the fingerprint's list count is a 32-bit word
    for count in (2 ** 31 - 1, -1):
        b = bytearray(blob)
        struct.pack_into("<i", b, secs["fingerprint"][1] + 20, count)
        refused(read_blob(harness, FULL, resum(bytes(b))), "section fingerprint", "overflows the section")
    # a count that fits the section but not the particle count, a tag beyond the particles, an entry count that is no multiple
    b = bytearray(blob)
    struct.pack_into("<Q", b, secs["particles"][1], 11)
    refused(read_blob(harness, FULL, resum(bytes(b))), "section particles")
    b = bytearray(blob)
    struct.pack_into("<i", b, secs["exclusions"][1] + 8, 12)
    refused(read_blob(harness, FULL, resum(bytes(b))), "section exclusions", "no two particles")
    b = bytearray(blob)
    n0 = struct.unpack_from("<Q", blob, secs["lists"][1] + 8)[0]
    struct.pack_into("<Q", b, secs["lists"][1] + 8, n0 - 1)
    refused(read_blob(harness, FULL, resum(bytes(b))), "section lists")


FIELDS = [("max_lists", 33, "CHEM_MAX_LISTS"), ("max_types", 15, "CHEM_MAX_TYPES"), ("max_reactions", 17, "CHEM_MAX_REACTIONS"), ("max_pot_params", 7, "CHEM_MAX_POT_PARAMS"),
          ("max_fix_sets", 9, "CHEM_MAX_FIX_SETS"), ("nlists", 5, "list count (blob 4, context 5)"), ("nlists", 3, "list count (blob 4, context 3)"),
          ("list.0.arity", 3, "list 0 arity"), ("list.2.kind", 21, "list 2 kind (blob 20, context 21)"), ("list.3.by_types", 0, "list 3 by_types"), ("list.0.hybrid", 0, "list 0 hybrid"),
          ("list.1.hybrid", 1, "list 1 hybrid"), ("n_reactions", 3, "reaction count (blob 2, context 3)"), ("n_dissociations", 0, "dissociation count"),
          ("n_fix_sets", 1, "fix-set count"), ("atrp_on", 0, "ATRP on"), ("npart", 13, "particle count (blob 12, context 13)")]


@pytest.mark.parametrize("field,value,named", FIELDS, ids=["%s=%d" % f[:2] for f in FIELDS])
def test_fingerprint_names_the_field_that_differs(harness, field, value, named):
    blob, _ = make_blob(harness, FULL, 8, "full")
    out = read_blob(harness, FULL, blob, seed=8, extra=["fpset %s %d" % (field, value)])
    refused(out, "the configuration differs", named)
    assert out[1] == "same 1"


def test_first_difference_wins(harness):
    blob, _ = make_blob(harness, FULL, 9, "full")
    out = read_blob(harness, FULL, blob, extra=["fpset npart 13", "fpset list.1.kind 11", "fpset atrp_on 0"])
    refused(out, "list 1 kind (blob 10, context 11)")
