"""The payloads that tests/test_deflate_model.py holds against zlib and tests/test_bgzf_deflate_gpu.py against the device."""
import os

import numpy as np

from tests import bam_model as B
from tests import fm_sam_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = np.random.default_rng(78).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
FIB_SEED = 5


def period(k, n, seed=3):
    unit = np.random.default_rng(seed).integers(0, 256, k, dtype=np.uint8).tobytes()
    return (unit * (n // k + 1))[:n]


def run(k):
    """a run of k equal bytes between random ones"""
    return RANDOM[:300] + b"\x41" * k + RANDOM[300:600]


def repeat_at(dist, total=65505):
    """64 random bytes at 700 and once more `dist` behind, zeros everywhere else: nothing between the two enters the hash table
    under the hashes of the 64 bytes, so the match is found exactly when the distance is allowed"""
    body = bytearray(total)
    piece = b"\x01" + RANDOM[1000:1062] + b"\x02"
    body[700:764] = piece
    body[700 + dist:764 + dist] = piece
    return bytes(body)


def fibonacci(seed=FIB_SEED):
    """byte b occurs fib(b + 1) times, 4180 bytes in all, shuffled"""
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    a = np.concatenate([np.full(c, b, np.uint8) for b, c in enumerate(fib)])
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def deep_tree(seed=5):
    """Eight rare bytes with the counts 1, 2, 3, 5, 8, 13, 21, 34 under 128 bytes that occur 100 times each, shuffled: nothing
    repeats, so every byte is a literal, and the rare ones hang as a chain below a leaf of the balanced part: 16 levels.  (The
    shuffled Fibonacci payload above does not get there: its frequent bytes repeat, matches take three quarters of it and the
    literal counts that are left give a tree of 10 levels.)"""
    counts = [1, 2, 3, 5, 8, 13, 21, 34] + [100] * 128
    a = np.concatenate([np.full(c, b, np.uint8) for b, c in enumerate(counts)])
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def text():
    with open(os.path.join(ROOT, "DESIGN.md"), "rb") as f:
        return f.read()[:65536]


def bam_records(qualities, want=120000, seed=11):
    """the unframed records of random batches, all with or all without qualities"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < want:
        b = S.random_batch(rng)
        if not b["ref_names"] or B.bad_reads_first(b):
            continue
        if (b["qual"] is not None) != qualities:
            continue
        got = B.bam_model(b)
        if "bam" in got:
            out.append(got["bam"])
            size += len(got["bam"])
    return b"".join(out)


def planted(rng):
    """random bytes of a random length with planted repeats"""
    n = int(rng.integers(1, 3000))
    a = bytearray(rng.integers(0, 256 if rng.random() < 0.5 else 4, n, dtype=np.uint8).tobytes())
    for _ in range(int(rng.integers(0, 6))):
        src, ln = int(rng.integers(0, n)), int(rng.integers(1, 600))
        dst = int(rng.integers(0, n))
        piece = bytes(a[src:src + ln])
        a[dst:dst + len(piece)] = piece
    return bytes(a[:n])


def short_cases():
    """name -> payload, each a few hundred bytes to a few thousand"""
    c = {"all 256 values": bytes(range(256)), "one byte": b"\x07", "one distance symbol": RANDOM[:40] + b"\x55" * 40,
         "no distance symbol": RANDOM[2000:2100], "fibonacci": fibonacci(), "deep tree": deep_tree()}
    for k in (2, 3, 255, 256, 257):
        c["period %d" % k] = period(k, 1500)
    for k in (257, 258, 259, 260, 516):
        c["run of %d" % k] = run(k)
    for n in (299, 300):
        c["zeros %d" % n] = bytes(n)
        c["ff %d" % n] = b"\xff" * n
    return c


def long_cases():
    c = {"zeros": bytes(65505), "ff": b"\xff" * 65281, "random": RANDOM[:65505], "text": text(), "period 257 long": period(257, 65505),
         "period 256 long": period(256, 65280)}
    for d in (32767, 32768, 32769):
        c["repeat at %d" % d] = repeat_at(d)
    c["records with qualities"] = bam_records(True)
    c["records without qualities"] = bam_records(False)
    return c
