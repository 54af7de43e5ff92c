#!/usr/bin/env python3
"""Generate tests/golden/ref_consensus_12.npz: the ground sets that the three builds of the reference under oracle/_ref
(eigen_f32, f32_packet4, exact_f64; fresh object per frame) give for frames 0..11 of tests/test_ref_consensus.py's set
(pwpp_synth.varied_frame(i)), as packed ground masks, with the md5 of every input frame.  The CPU test of the consensus
harness holds the restatement against these where oracle/_ref has not been built.  Needs oracle/_ref (make -C oracle ref)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "patchwork-plusplus_amd", "python"))
import oracle_lib as ol  # noqa: E402
import pwpp_synth  # noqa: E402

FLAVOURS = (("eigen_f32", ol.ARITH_EIGEN_F32), ("f32_packet4", ol.ARITH_F32_PACKET4), ("exact_f64", ol.ARITH_EXACT_F64))
FRAMES = 12


def main():
    ol.build()
    out = {"md5": [], "n_points": []}
    for i in range(FRAMES):
        pts = pwpp_synth.varied_frame(i)
        out["md5"].append(hashlib.md5(pts.tobytes()).hexdigest())
        out["n_points"].append(pts.shape[0])
        for name, arith in FLAVOURS:
            lib = ol.reference(arith)
            assert lib is not None, "build oracle/_ref first (make -C oracle ref)"
            mask = np.zeros(pts.shape[0], np.uint8)
            mask[ol.Estimator(lib, arith=arith).run(pts).ground_idx] = 1
            out["%s/%d" % (name, i)] = np.packbits(mask)
    out["md5"], out["n_points"] = np.array(out["md5"]), np.array(out["n_points"], np.int64)
    np.savez_compressed(os.path.join(HERE, "ref_consensus_12.npz"), **out)


if __name__ == "__main__":
    main()
