"""Per-launch table of MobileNet-v2's 17 depthwise convs from a rocprofv3 kernel trace of tools/mobilenet_bench.py:
compulsory bytes (input + output + residual, channel-quad tensors), median duration over the traced forwards, and the fraction of
6.3 TB/s that is.
    python tools/mobilenet_dw_digest.py <kernel_trace.csv> [--batch 32] [--size 224]"""
import argparse
import csv
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from planer_amd.irgen.mobilenetv2 import SETTING  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def dw_layers(n, size):
    """-> [(block, C, H, stride, bytes)] in forward order (the stem halves the map; residuals never land on a depthwise conv)."""
    out, cin, h, bi = [], 32, (size + 1) // 2, 0
    for t, c, reps, s in SETTING:
        for i in range(reps):
            st = s if i == 0 else 1
            hid = cin * t
            ho = (h - 1) // st + 1
            cq = (hid + 3) // 4 * 4
            out.append(("b%d" % bi, hid, h, st, 4 * n * cq * (h * h + ho * ho)))
            cin, h, bi = c, ho, bi + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    rows = list(csv.DictReader(open(args.trace)))
    dw = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows
                 if "conv_dw_kernel" in r["Kernel_Name"] and "float, 4" in r["Kernel_Name"]))
    layers = dw_layers(args.batch, args.size)
    k = len(layers)
    if not dw or len(dw) % k:
        sys.exit("%d channel-quad depthwise launches in the trace: not a whole number of %d-conv forwards" % (len(dw), k))
    forwards = [dw[i:i + k] for i in range(0, len(dw), k)]
    print("| block | C | map | stride | compulsory MB | median us | TB/s | of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|")
    tot_b = tot_t = 0.0
    for j, (blk, c, h, s, nbytes) in enumerate(layers):
        ts = sorted((f[j][1] - f[j][0]) * 1e-9 for f in forwards)
        t = ts[len(ts) // 2]
        tot_b += nbytes
        tot_t += t
        print("| %s | %d | %dx%d | %d | %.1f | %.1f | %.2f | %.2f |" % (blk, c, h, h, s, nbytes / 1e6, t * 1e6, nbytes / t / 1e12,
                                                                      nbytes / t / HBM_BYTES_PER_S))
    print("| all 17 | | | | %.1f | %.1f | %.2f | %.2f |" % (tot_b / 1e6, tot_t * 1e6, tot_b / tot_t / 1e12,
                                                            tot_b / tot_t / HBM_BYTES_PER_S))
    print("\n(%d traced forwards of batch %d, %dx%d)" % (len(forwards), args.batch, args.size, args.size))


if __name__ == "__main__":
    main()
