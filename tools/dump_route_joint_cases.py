#!/usr/bin/env python3
"""Dump cases of tests/route_joint_cases.py, with tests/route_joint_ref.py's answers, into the
binary file tools/san_route_joint.cpp reads (little endian):
  "UAMJ0001", int32 n_cases, then per case
  int32 nx, ny; float64 x0, y_top, dx, dy, lam; uint32 block_flags; int32 inflate, G, Q, N, S;
  rec [ny][nx][4] u32; goals [G][2] f64; starts [Q][2] f64;
  dist [ny][nx] f64; next [ny][nx] u8; owner [ny][nx] i32;
  S times: int32 span; wp [Q][N+2][2] f64; status, steps, vertices, goal [Q] i32 each.

usage: python tools/dump_route_joint_cases.py OUT [case ...]   (default: the cases named in
       route_joint_cases.SANITIZE)"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import route_joint_cases as JC  # noqa: E402

SPANS = (0, 1, 7, 64)


def main():
    out, names = sys.argv[1], sys.argv[2:] or list(JC.SANITIZE)
    with open(out, "wb") as f:
        f.write(b"UAMJ0001" + struct.pack("<i", len(names)))
        for name in names:
            c, r = JC.BY_NAME[name], JC.reference(name)
            g = c["geo"]
            f.write(struct.pack("<ii5dIi4i", g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy, c["lam"],
                                c["block_flags"], c["inflate"], len(c["goals"]),
                                len(c["starts"]), c["N"], len(SPANS)))
            f.write(np.ascontiguousarray(c["rec"]).view("<u4").tobytes())
            f.write(c["goals"].astype("<f8").tobytes())
            f.write(c["starts"].astype("<f8").tobytes())
            f.write(r["dist"].astype("<f8").tobytes())
            f.write(r["next"].astype("u1").tobytes())
            f.write(r["owner"].astype("<i4").tobytes())
            for span in SPANS:
                p = JC.reference_paths(name, span)
                f.write(struct.pack("<i", span))
                f.write(p["wp"].astype("<f8").tobytes())
                for k in ("status", "steps", "vertices", "goal"):
                    f.write(p[k].astype("<i4").tobytes())
    print(out, os.path.getsize(out), "bytes,", len(names), "cases:", " ".join(names))


if __name__ == "__main__":
    main()
