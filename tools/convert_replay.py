#!/usr/bin/env python3
"""Rewrites a replay store in the other record format: the reference's (fp32 arrays in msgpack) or the compact one
(nextbestpath_amd/utility/replay_codec.py; lossless).  Host only -- the numpy codec, no GPU -- and keys and order are kept, so

    convert_replay.py SRC TMP --to compact && convert_replay.py TMP DST --to reference

reproduces every value of a reference-format SRC byte for byte.  Records already in the target format are copied as they are.

    python tools/convert_replay.py SRC DST --to compact|reference
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def convert(src, dst, to):
    """-> (records, bytes read, bytes written).  DST gets SRC's container: the append-only log for a log, else LMDB's format."""
    from nextbestpath_amd.utility import nbp_utils as nu
    nu.check_replay_format(to)
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("convert_replay: SRC and DST are the same store")
    if not os.path.isdir(src):
        raise FileNotFoundError(src)
    env_in = nu.open_experience_db(src)
    env_out = nu.LogEnv(dst) if isinstance(env_in, nu.LogEnv) else nu.open_experience_db(dst)
    if env_out.entries():
        raise ValueError(f"convert_replay: {dst} already holds records")
    n = b_in = b_out = 0
    for key, value in env_in.items():
        rec = nu.unpack_record(value, keep_compact=True)
        have = "compact" if "nbpc" in rec else "reference"
        out = value if have == to else nu.pack_record(rec, to)
        env_out.put(key, out)
        n, b_in, b_out = n + 1, b_in + len(value), b_out + len(out)
    env_in.close()
    env_out.close()
    return n, b_in, b_out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--to", required=True, choices=("compact", "reference"))
    a = ap.parse_args()
    n, b_in, b_out = convert(a.src, a.dst, a.to)
    print(f"{n} records: {b_in} -> {b_out} value bytes ({b_in / max(b_out, 1):.2f}x)")


if __name__ == "__main__":
    main()
