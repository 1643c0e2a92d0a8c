"""Writes tests/golden/read_chunks_cases.json: what the reference's own ``read_chunks`` / ``ReadChunk`` (bonito/reader.py) yield for
ramp signals of the lengths around one chunk and one and two strides beyond it.

    python tests/golden/make_golden_read_chunks.py <path to the reference's bonito/reader.py>

The reference module is loaded from its file (it imports torch and numpy only at module level). The signal of a case is
0, 1, 2, ... as float32, so a chunk is described completely by its first sample and its length. Only the JSON of inputs and
recorded values is committed. Needs no GPU; run it where the reference is."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

READ = dict(read_id="7d5a3c1e-read", run_id="run_a1", filename="batch_0.pod5", mux=3, channel=12, start=101.25, duration=2.5)
CHUNKSIZE, OVERLAP = 1000, 100
STEP = CHUNKSIZE - OVERLAP
LENGTHS = [0, CHUNKSIZE - 1, CHUNKSIZE, CHUNKSIZE + 1, CHUNKSIZE + STEP - 1, CHUNKSIZE + STEP, CHUNKSIZE + STEP + 1,
           CHUNKSIZE + 2 * STEP - 1, CHUNKSIZE + 2 * STEP, CHUNKSIZE + 2 * STEP + 1, 5 * CHUNKSIZE + 37]
OTHER = [(4000, 400, 12345), (7, 0, 30), (7, 6, 30), (10, 3, 10)]               # (chunksize, overlap, length)


def main():
    spec = importlib.util.spec_from_file_location("reference_reader", sys.argv[1])
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cases = []
    for chunksize, overlap, length in [(CHUNKSIZE, OVERLAP, n) for n in LENGTHS] + OTHER:
        read = types.SimpleNamespace(signal=np.arange(length, dtype=np.float32), **READ)
        chunks = list(ref.read_chunks(read, chunksize=chunksize, overlap=overlap))
        cases.append(dict(chunksize=chunksize, overlap=overlap, length=length, ids=[c.read_id for c in chunks],
                          first=[int(c.signal[0]) for c in chunks], sizes=[int(len(c.signal)) for c in chunks],
                          fields=[[c.run_id, c.filename, c.mux, c.channel, c.start, c.duration, c.template_start, c.template_duration]
                                  for c in chunks[:1]]))
        for c in chunks:
            assert np.array_equal(c.signal, read.signal[int(c.signal[0]):int(c.signal[0]) + chunksize])
    with open(os.path.join(HERE, "read_chunks_cases.json"), "w") as fh:
        json.dump(dict(read=READ, cases=cases), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
