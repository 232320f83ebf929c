"""Generate tests/golden/gguf/ggml-vocab-*.gguf — the GGUF files the reference ships under models/
(real llama.cpp output, metadata only, no tensors) as fixtures of tests/test_gguf.py.

A file that fits the repository's 1 MiB limit is copied whole. A larger one is copied with every
metadata array (tokens, scores, token types, merges) cut to its first KEEP elements: the bytes of
everything kept are the file's own, only the arrays' element counts change. Run:
    python tests/golden/make_gguf_vocab.py <the reference's models/ directory>
"""
import glob
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1 << 20
KEEP = 2048
STRING, ARRAY = 8, 9
SIZE = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 1, 10: 8, 11: 8, 12: 8}  # GGUF scalar value types
ALIGN = 32


def _after(data, t, p):
    """Offset just past the value of type t (not ARRAY) at p."""
    if t == STRING:
        return p + 8 + struct.unpack_from("<Q", data, p)[0]
    return p + SIZE[t]


def cut_arrays(data, keep):
    version, n_t, n_kv = struct.unpack_from("<IQQ", data, 4)
    assert data[:4] == b"GGUF" and version == 3 and n_t == 0, "a tensor-less GGUF v3 file is expected"
    out = bytearray(data[:24])
    p = 24
    for _ in range(n_kv):
        q = _after(data, STRING, p)  # the key
        t = struct.unpack_from("<I", data, q)[0]
        q += 4
        if t != ARRAY:
            q = _after(data, t, q)
            out += data[p:q]
        else:
            et, n = struct.unpack_from("<IQ", data, q)
            out += data[p:q + 4] + struct.pack("<Q", min(n, keep))
            q += 12
            first, kept_end = q, None
            for i in range(n):
                if i == keep:
                    kept_end = q
                q = _after(data, et, q)
            out += data[first:q if kept_end is None else kept_end]
        p = q
    assert all(b == 0 for b in data[p:]), "only padding may follow the metadata"
    out += b"\0" * (-len(out) % ALIGN)
    return bytes(out)


def main(src):
    dst = os.path.join(HERE, "gguf")
    os.makedirs(dst, exist_ok=True)
    for path in sorted(glob.glob(os.path.join(src, "ggml-vocab-*.gguf"))):
        data = open(path, "rb").read()
        how = "whole"
        if len(data) > LIMIT:
            data, how = cut_arrays(data, KEEP), f"arrays cut to {KEEP}"
        assert len(data) <= LIMIT
        with open(os.path.join(dst, os.path.basename(path)), "wb") as f:
            f.write(data)
        print(f"{os.path.basename(path)}: {len(data)} B ({how})")


if __name__ == "__main__":
    main(sys.argv[1])
