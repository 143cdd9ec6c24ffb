"""Records what the reference's own shader headers answer: tests/golden/reference_pin.npz.

Needs oracle/_ref/libmetal_ref.so (`make -C oracle` where the reference is present) and calls only its ref_* entry points
(oracle/pin_api.h) on the inputs of tests/reference_pin_cases.py.  Per case the file keeps
  crc/<case>    CRC-32 of the compared fields of the WHOLE batch (edges + 200 000 seeded; inputs are regenerated, not stored),
                bits side by side, every NaN as 0x7FC00000 (reference_pin_cases.canonical);
  head/<case>   those bits for the hand-made edge inputs and the first 512 seeded ones, to show WHERE a CRC went wrong;
and for the scenes of tests/test_gpu_reference_pin.py, crc/trc/<scene> and crc/trc_any/<scene>: the CRC-32 of Scene::hit's records
of 8 192 rays as trc_hit reports them (the record only where the answer is yes; the first 512 are in head/scene_<scene>).
Fields the reference leaves unwritten (the table of tests/test_reference_pin.py) are not part of either.

    python tests/golden/make_reference_pin.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import reference_pin_cases as rc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

OUT = os.path.join(HERE, "reference_pin.npz")


def crc(bits):
    return np.uint32(zlib.crc32(np.ascontiguousarray(bits).tobytes()))


def main():
    ref = po.Pin(ref=True)
    assert ref.literal_probe(np.float32(0.1), np.float32(0.7)) == np.float32(1.0) - np.float32(0.1) - np.float32(0.7), "literals are not float"
    out = {}
    for name, case in rc.build_cases().items():
        fields = case.run(ref)
        bits = rc.canonical(fields, case.excluded)
        out[f"crc/{name}"], out[f"n/{name}"] = crc(bits), np.int64(len(bits))
        out[f"head/{name}"] = bits[case.stored[case.stored < len(bits)]]
        if name.startswith("scene_") and name.split("scene_any_")[-1].split("scene_")[-1] in rc.GPU_SCENES:
            view = rc.canonical(rc.trc_view(fields["accepted"], fields))
            key = name.replace("scene_any_", "trc_any/").replace("scene_", "trc/")
            out[f"crc/{key}"] = crc(view)
            if "_any_" in name:      # the production walk of any-hit rays defines the answer alone
                out[f"crc/hit_any_{name[len('scene_any_'):]}"] = crc(view[:, 0])
        print(f"{name:36s} {len(bits):7d} inputs  crc {int(out['crc/' + name]):08x}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
