"""Generate tests/golden/hash_collisions.json — pairs of different byte strings
of equal length with the same 64-bit word_hash (emqx_amd/csrc/egm_common.h).

    python tests/golden/make_hash_collisions.py

word_hash folds 4-byte little-endian chunks with h = (h ^ c) * FNV_PRIME and
mixes (with the length) only at the end, so two inputs of equal length that
reach the same 64-bit state collide whatever follows.  A chunk only touches
the low 32 bits of the state before the multiply, so

  1. a birthday search over two random chunks finds inputs whose states agree
     in the high 32 bits (4 M samples -> ~2 000 such pairs);
  2. a third chunk each, c and c ^ (low-half difference), cancels the low 32
     bits — possible when every byte of the difference is the XOR of two
     alphabet characters.

The search starts from the state after the class's shared prefix (a state
difference is not invariant under a change of the starting state: the fold
mixes XOR with a multiply), so every class with another prefix has its own
search.  A shared tail after the three chunks keeps a pair colliding.

Everything is integer arithmetic on a counter-based generator (splitmix64 of
the sample index), so the output does not depend on numpy's random streams:
running this again reproduces the committed file byte for byte.

Classes (each PAIRS pairs; alphabet [A-Za-z0-9_-] only):
  w12       12-byte words                          (inline compare)
  w16       4-byte shared prefix + 12              (inline boundary)
  w17       the same + 1 shared tail byte          (blob compare, inline bytes differ)
  w28..w31  16-byte shared prefix + 12 + 0..3 tail (inline bytes identical)
  f         whole filters a/b/<12 bytes>/x         (the host filter store)
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hash_collisions.json")

ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-"
FNV_BASIS = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
M64 = (1 << 64) - 1
SAMPLES = 1 << 22
PAIRS = 4
SEED = 0x45474D5F48415348   # "EGM_HASH"


def mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def fold(h, data):
    """The state after folding `data` (the last chunk zero-padded) into h."""
    for i in range(0, len(data), 4):
        h = ((h ^ int.from_bytes(data[i:i + 4], "little")) * FNV_PRIME) & M64
    return h


def word_hash(data):
    return mix64(fold(FNV_BASIS, data) ^ ((len(data) & 0xFF) << 56))


def splitmix(idx, seed):
    with np.errstate(over="ignore"):
        z = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def xor_table():
    """d -> the first alphabet byte a with a ^ d in the alphabet too (d < 256)."""
    t = {}
    for a in ALPHABET:
        for b in ALPHABET:
            t.setdefault(a ^ b, a)
    return t


def search(prefix, seed, want):
    """`want` pairs of 12-byte strings that collide after `prefix` (a multiple of 4 bytes)."""
    assert len(prefix) % 4 == 0
    h0 = np.uint64(fold(FNV_BASIS, prefix))
    al = np.frombuffer(ALPHABET, np.uint8).astype(np.uint64)
    r0 = splitmix(np.arange(SAMPLES, dtype=np.uint64), seed)
    r1 = splitmix(np.arange(SAMPLES, dtype=np.uint64), seed ^ 0x5555555555555555)
    chunks = []
    for r in (r0, r1):   # 8 alphabet bytes = 48 random bits: a chunk from each word's halves
        c = np.zeros(SAMPLES, np.uint64)
        for k in range(4):
            c |= al[(r >> np.uint64(6 * k)) & np.uint64(63)] << np.uint64(8 * k)
        chunks.append(c)
    with np.errstate(over="ignore"):
        h = (h0 ^ chunks[0]) * np.uint64(FNV_PRIME)
        h = (h ^ chunks[1]) * np.uint64(FNV_PRIME)
    hi = h >> np.uint64(32)
    order = np.argsort(hi, kind="stable")
    same = np.nonzero(hi[order][1:] == hi[order][:-1])[0]
    xt = xor_table()
    out = []
    for k in same.tolist():
        i, j = int(order[k]), int(order[k + 1])
        if chunks[0][i] == chunks[0][j] and chunks[1][i] == chunks[1][j]:
            continue
        d = (int(h[i]) ^ int(h[j])) & 0xFFFFFFFF
        db = d.to_bytes(4, "little")
        if any(x not in xt for x in db):
            continue
        ca = bytes(xt[x] for x in db)
        cb = bytes(xt[x] ^ x for x in db)
        a = int(chunks[0][i]).to_bytes(4, "little") + int(chunks[1][i]).to_bytes(4, "little") + ca
        b = int(chunks[0][j]).to_bytes(4, "little") + int(chunks[1][j]).to_bytes(4, "little") + cb
        assert a != b and word_hash(prefix + a) == word_hash(prefix + b)
        out.append((a, b))
        if len(out) == want:
            return out
    raise SystemExit("too few collisions: raise SAMPLES")


def build():
    p4, p16 = b"Wp4_", b"shared-prefix_16"
    assert len(p4) == 4 and len(p16) == 16
    classes = {}
    classes["w12"] = search(b"", SEED, PAIRS)
    s4 = search(p4, SEED + 1, PAIRS)
    classes["w16"] = [(p4 + a, p4 + b) for a, b in s4]
    classes["w17"] = [(p4 + a + b"t", p4 + b + b"t") for a, b in s4]
    s16 = search(p16, SEED + 2, PAIRS)
    for k, tail in enumerate((b"", b"u", b"uv", b"uvw")):
        classes["w%d" % (28 + k)] = [(p16 + a + tail, p16 + b + tail) for a, b in s16]
    classes["f"] = [(b"a/b/" + a + b"/x", b"a/b/" + b + b"/x") for a, b in search(b"a/b/", SEED + 3, PAIRS)]
    for name, pairs in classes.items():
        for a, b in pairs:
            assert a != b and len(a) == len(b) and word_hash(a) == word_hash(b), (name, a, b)
            if name != "f":
                assert len(a) == int(name[1:]) and all(x in ALPHABET for x in a + b)
    return {"alphabet": ALPHABET.decode(), "classes": {n: [[a.decode(), b.decode()] for a, b in p]
                                                       for n, p in classes.items()}}


def main():
    doc = build()
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT, {n: len(p) for n, p in doc["classes"].items()})


if __name__ == "__main__":
    main()
