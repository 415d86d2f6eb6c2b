#!/usr/bin/env python3
"""Writes tests/golden/ref_writer_pins.json: what the REFERENCE's own writers make of the synthetic cases of the xtc / trr
writer and decoder tests -- the sha256 of each file written by its vendored C xdrfile (compiled where it lies by
oracle/Makefile into oracle/_ref, build container only) and of the coordinates its reader decodes from it (float32, C order).
The tests compare the library's encoder and decoder against these pins wherever they run, and against the reference's
compiled code as well where oracle/_ref exists.

    python tests/golden/make_ref_writer_pins.py"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_trr_reader as TT              # noqa: E402
import test_xtc_decoder as TD             # noqa: E402
import test_xtc_writer as TW              # noqa: E402


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    pins = {"xtc_decoder": {}, "xtc_writer": {}, "xtc_random": {}, "trr_writer": {}}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "f")
        for case in TD.DECODER_CASES:
            frames, box, prec = TD.decoder_case(case)
            TD.write_with_ref(p, frames, box, prec)
            pins["xtc_decoder"][case] = {"file_sha256": sha(p), "decode_sha256": TD.sha256_bytes(TD.read_with_ref(p, frames[0].shape[0]).tobytes())}
        for case in TW.SAME_BYTES_CASES:
            frames, box, prec = TW.same_bytes_case(case)
            if case == "no_box_nan":
                for f in frames:
                    f[5] = 0.0                     # the atom the library is handed without position (NaN x) is written as the origin
            TD.write_with_ref(p, frames, box, prec)
            pins["xtc_writer"][case] = sha(p)
        for seed in range(48):
            frames, box, prec = TW.random_case(seed)
            TD.write_with_ref(p, frames, box, prec)
            pins["xtc_random"][str(seed)] = {"file_sha256": sha(p), "decode_sha256": TD.sha256_bytes(TD.read_with_ref(p, frames[0].shape[0]).tobytes())}
        for seed in range(6):
            frames, box = TT.writer_case(seed)
            TT.write_trr_with_ref(p, frames, box)
            pins["trr_writer"][str(seed)] = sha(p)
    json.dump(pins, open(TD.REF_PINS, "w"), indent=1, sort_keys=True)
    print({k: len(v) for k, v in pins.items()})


if __name__ == "__main__":
    main()
