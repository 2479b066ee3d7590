"""The one chain clock (voxgraph_amd/csrc/vgx_chain_clock.h) without a GPU: tests/cpp/chain_clock_check.cpp includes that
header alone, is built with AddressSanitizer and UBSan as a program of its own and prints every take of a set of sequences;
here every line is recomputed from the stated rule:

  * the epoch of a launch is the one before plus 1; after a launch at Max = 2^30 - 1 the next one has clear_first and
    epoch 1; no other launch has clear_first
  * an epoch is never 0 and never above Max (the tag is 30 bits of the tile word: a larger one shifts out)
  * ticket_base is the starting tickets plus every earlier launch's tiles, modulo 2^32
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = (1 << 30) - 1
WRAP = 1 << 32


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    cxx = shutil.which("g++")                                         # the compiler the library's own Makefile names
    assert cxx is not None
    exe = str(tmp_path_factory.mktemp("chain_clock") / "chain_clock_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "voxgraph_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "chain_clock_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stderr)
    assert out.returncode == 0 and "chain_clock_check ok" in out.stdout and "ERROR" not in out.stderr
    seqs = []
    for line in out.stdout.splitlines():
        tok = line.split()
        if tok[0] == "S":
            seqs.append({"name": tok[1], "epoch": int(tok[2]), "tickets": int(tok[3]), "takes": []})
        elif tok[0] == "T":
            seqs[-1]["takes"].append(dict(zip(("tiles", "epoch", "base", "clear", "epoch_after", "tickets_after"), map(int, tok[1:]))))
    assert len(seqs) >= 20 and all(s["takes"] for s in seqs)
    return seqs


def named(seqs, name):
    got = [s for s in seqs if s["name"] == name]
    assert got, name
    return got


def test_epochs_count_up_from_a_new_handle(sequences):
    (s,) = named(sequences, "fresh")
    assert (s["epoch"], s["tickets"]) == (0, 0)
    assert [t["epoch"] for t in s["takes"]] == list(range(1, len(s["takes"]) + 1))
    assert not any(t["clear"] for t in s["takes"])
    # the tile counts the issue names are all there
    assert {1, 64, 65, 1 << 24, 1 << 31} <= {t["tiles"] for t in s["takes"]}


def test_the_rollover_clears_once_and_restarts_at_one(sequences):
    (s,) = named(sequences, "rollover")
    assert s["epoch"] == MAX - 1
    t = s["takes"]
    assert (t[0]["epoch"], t[0]["clear"]) == (MAX, 0)
    assert (t[1]["epoch"], t[1]["clear"]) == (1, 1)
    assert [(x["epoch"], x["clear"]) for x in t[2:]] == [(k, 0) for k in range(2, len(t))]
    (s,) = named(sequences, "at_max")
    assert s["epoch"] == MAX and (s["takes"][0]["epoch"], s["takes"][0]["clear"]) == (1, 1)


def test_every_take_follows_the_stated_rule(sequences):
    rolled = 0
    for s in sequences:
        epoch, launched = s["epoch"], 0
        for t in s["takes"]:
            want_clear = epoch == MAX
            want_epoch = 1 if want_clear else epoch + 1
            assert (t["epoch"], t["clear"]) == (want_epoch, int(want_clear)), (s["name"], t)
            assert 1 <= t["epoch"] <= MAX
            assert t["epoch_after"] == t["epoch"]
            # the sum of all earlier tiles, as an integer of any size, reduced once
            assert t["base"] == (s["tickets"] + launched) % WRAP, (s["name"], t)
            launched += t["tiles"]
            assert t["tickets_after"] == (s["tickets"] + launched) % WRAP
            epoch = t["epoch"]
            rolled += t["clear"]
    # every seeded sequence starts within 12 launches of the rollover and makes 24
    assert rolled >= 16 + 3


def test_a_take_may_straddle_two_to_the_32(sequences):
    (s,) = named(sequences, "straddle")
    assert s["tickets"] == WRAP - 30
    a, b = s["takes"]
    assert (a["tiles"], a["base"], a["tickets_after"]) == (68, WRAP - 30, 38)
    assert (b["base"], b["tickets_after"]) == (38, 106)
    # what the device computes for the k-th workgroup of the straddling launch: (u32)(ticket word) - base = k
    for k in (0, 29, 30, 67):
        assert ((a["base"] + k) % WRAP - a["base"]) % WRAP == k
    (s,) = named(sequences, "exact")
    assert [t["base"] for t in s["takes"]] == [WRAP - 68, 0]
    (s,) = named(sequences, "halves")
    assert [t["base"] for t in s["takes"]] == [1 << 31, 0, 1 << 31, (1 << 31) - 1]
    # the seeded sequences wrap too
    wrapped = [s for s in named(sequences, "seeded") if any(t["tickets_after"] < t["base"] for t in s["takes"])]
    assert len(wrapped) >= 8
