#!/usr/bin/env python3
"""Dump cases of tests/route3d_joint_cases.py, with tests/route3d_joint_ref.py's answers, into the
binary file tools/san_route3d_joint.cpp reads (little endian):
  "UAMVJ001", int32 n_cases, then per case
  int32 nx, ny, nz; float64 x0, y_top, dx, dy, z0, dz, lam; uint32 block_flags; int32 inflate;
  float64 agl, kappa; int32 G, Q, N, S, W;
  vol [W] u32 (the volume buffer's words: voxels, then the columns at the 256-B aligned offset);
  goals [G][3] f64; starts [Q][3] f64;
  dist [ny][nx][nz] f64; next [ny][nx][nz] u8; owner [ny][nx][nz] i32;
  S times: int32 span; wp3 [Q][N+2][3] f64; status, steps, vertices, goal [Q] i32 each.

usage: python tools/dump_route3d_joint_cases.py OUT [case ...]   (default: the cases named in
       route3d_joint_cases.SANITIZE)"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import route3d_cases as C  # noqa: E402
import route3d_joint_cases as JC  # noqa: E402


def main():
    out, names = sys.argv[1], sys.argv[2:] or list(JC.SANITIZE)
    with open(out, "wb") as f:
        f.write(b"UAMVJ001" + struct.pack("<i", len(names)))
        for name in names:
            c, r = JC.BY_NAME[name], JC.reference(name)
            g = c["geo"]
            vol = C.volume_words(c)
            f.write(struct.pack("<3i7dIi2d5i", g.nx, g.ny, g.nz, g.x0, g.y_top, g.dx, g.dy, g.z0,
                                g.dz, c["lam"], c["block_flags"], c["inflate"], c["agl"],
                                c["kappa"], len(c["goals"]), len(c["starts"]), c["N"],
                                len(JC.SPANS), vol.size))
            f.write(vol.astype("<u4").tobytes())
            f.write(c["goals"].astype("<f8").tobytes())
            f.write(c["starts"].astype("<f8").tobytes())
            f.write(r["dist"].astype("<f8").tobytes())
            f.write(r["next"].astype("u1").tobytes())
            f.write(r["owner"].astype("<i4").tobytes())
            for span in JC.SPANS:
                p = JC.reference_paths(name, span)
                f.write(struct.pack("<i", span))
                f.write(p["wp3"].astype("<f8").tobytes())
                for k in ("status", "steps", "vertices", "goal"):
                    f.write(p[k].astype("<i4").tobytes())
    print(out, os.path.getsize(out), "bytes,", len(names), "cases:", " ".join(names))


if __name__ == "__main__":
    main()
