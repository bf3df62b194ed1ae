"""C2-size timing of a tuner whose receivers have an audio filter of 64 / 128 / 256 taps: us per block through the streaming
launch or with a kernel launch per block (development aid; bench.py is the contract).  profiles/stream_long_audio.txt was
taken with it.

  python tools/stream_long_audio_time.py --l2 128 --stream 1 [--blocks 400] [--windows 8] [--d2 5] [--root DIR]

--root: the checkout whose webradio_amd package (and built library) is measured -- this one by default; another commit's
build for a comparison on the same box, one process per figure, the two alternating.  Prints one JSON line: the median,
the smallest and the largest of the windows' us per block, and what stream_info() said."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--l2", type=int, default=64, choices=(64, 128, 256))
ap.add_argument("--stream", type=int, default=1)
ap.add_argument("--blocks", type=int, default=400)       # per window: one streaming launch takes up to WR_STREAM_MAX_BLOCKS
ap.add_argument("--windows", type=int, default=8)
ap.add_argument("--d2", type=int, default=5)            # audio decimation off C2's 250 k channel rate
ap.add_argument("--resident", type=int, default=12)     # input blocks cycled through: more than the Infinity Cache holds
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch                                              # noqa: E402
from webradio_amd import capi, synth                      # noqa: E402
from webradio_amd.device import Device, Tuner             # noqa: E402

c2 = synth.C2
fs, n, crate = c2["input_rate"], c2["block_frames"], c2["chan_rate"]
assert crate % args.d2 == 0
ifs = synth.c2_ifs(256)
dev = Device(0, torch.cuda.current_stream().cuda_stream)
xs = synth.fm_stream_torch(n * args.resident, fs, ifs[::4], "cuda")
blocks = [xs[2 * n * b: 2 * n * (b + 1)] for b in range(args.resident)]
torch.cuda.synchronize()
t = Tuner(dev, fs, 256, n, capi.WR_NCO_ROTATE)
for f in ifs:
    t.add_receiver(f, c2["chan_passband"], crate, capi.WR_FM, c2["audio_passband"], crate // args.d2,
                   fir_lengths=(64, args.l2))
t.streaming(bool(args.stream))


def window(count):
    t0 = time.perf_counter()
    for i in range(count):
        t.submit_device(blocks[i % args.resident], n)
    t.flush()                                             # closes the streaming launch / sends the last post stage
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / count


window(args.blocks)                                       # every shape the timed windows use, once
window(args.blocks)
opened0 = t.stream_info()
us = [window(args.blocks) for _ in range(args.windows)]
info = t.stream_info()
t.destroy()
print(json.dumps({"label": args.label, "l2": args.l2, "d2": args.d2, "asked_to_stream": bool(args.stream),
                  "launches": info[1] - opened0[1], "streamed_blocks": info[2] - opened0[2],
                  "blocks_per_window": args.blocks, "windows": args.windows,
                  "us_per_block_median": round(statistics.median(us), 2), "us_per_block_min": round(min(us), 2),
                  "us_per_block_max": round(max(us), 2)}), flush=True)
