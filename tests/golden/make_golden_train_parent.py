"""Writes tests/golden/train_parent.json: the buffer sizes of the training layers BEFORE the reduction over rows, the GEMM row loop
and the small helpers of csrc/lstm_train.hip and csrc/train_layers.hip were written once (csrc/train_common.h, csrc/train_common.hip).

    git checkout 5ee63b5 && python build.py && python tests/golden/make_golden_train_parent.py 5ee63b5

It needs no GPU: the size functions are host code. The partial sums of the weight gradients are the tail of every workspace, so the
sizes pin how the rows are split (ceil(M / 512) blocks, at most 1024 / tiles, rows rounded up to 32; the bias: ceil(M / 256), at
most 1024), which is the order of the sums. The LSTM table holds shapes where the cap binds (H = 1024: one block) and where the last
block is short (150 x 20 at H = 64: six blocks of 512 rows, the last with 440). A convolution whose Cin is neither 1 nor a multiple
of 8 is recorded as the library answers it (0: refused) and with the channels padded to 8, as train_ops.conv1d serves it.
tests/test_train_layers_ref_cpu.py asserts that the present library reproduces every row."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

LSTM_H = (32, 64, 96, 128, 384, 1024)
LSTM_TN = ((1, 1), (37, 5), (150, 20), (600, 5), (600, 64))


def main():
    from bonito_amd import _lib
    from train_layers_ref import CONV_CASES, LINEAR_CASES
    lib = _lib.lib()
    lstm = [[T, N, H, lib.bh_lstm_train_saved_bytes(T, N, H), lib.bh_lstm_train_backward_workspace(T, N, H)]
            for H in LSTM_H for T, N in LSTM_TN]
    conv = []
    for N, Cin, Cout, K, stride, Lin in CONV_CASES:
        for c in sorted({Cin, Cin if Cin == 1 else (Cin + 7) // 8 * 8}):
            conv.append([N, Lin, c, Cout, K, stride, K // 2, lib.bh_conv1d_train_workspace(N, Lin, c, Cout, K, stride, K // 2)])
    linear = [[T, N, K, C, lib.bh_linear_train_workspace(T, N, K, C)] for T, N, K, C in (c[:4] for c in LINEAR_CASES)]
    assert all(r[3] and r[4] for r in lstm) and all(r[4] for r in linear) and all(r[7] for r in conv if r[2] == 1 or r[2] % 8 == 0)
    with open(os.path.join(HERE, "train_parent.json"), "w") as fh:
        json.dump(dict(parent=sys.argv[1], lstm=lstm, conv=conv, linear=linear), fh, separators=(",", ":"))
        fh.write("\n")
    print("%d lstm, %d conv, %d linear rows" % (len(lstm), len(conv), len(linear)))


if __name__ == "__main__":
    main()
