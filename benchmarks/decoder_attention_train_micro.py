"""Microseconds per forward + backward of the decoder layer's self-attention block under autograd (in-projection to
out-projection, `SalienceTransformerDecoderLayer._self_attention_train`) on its two training forms: "torch"
(`nn.MultiheadAttention` with the boolean mask) and "hip" (two projection GEMMs, `attention_train.attention_qk_v_masked`,
out-projection; csrc/attention_train_masked.hip), on the same device and in the same process.

    python benchmarks/decoder_attention_train_micro.py [--repeats 9] [--iters 200] [--out FILE.json]

B = 2, E = 256, H = 8, N in {900, 1100, 1500} rows with the denoising mask of that row count (900: no targets, nothing
masked; 1100: 50 groups of 2 x 2; 1500: one group of 2 x 300).  Per row count the two forms alternate window by window;
a window is ``--iters`` calls between two device events after a warm-up of both forms; the figure is the median over
``--repeats`` windows, with the fastest and the slowest window next to it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, E, H, NQ = 2, 256, 8, 900
CONFIGS = {900: (0, 1), 1100: (2, 50), 1500: (300, 1)}     # rows -> (max_gt, denoising groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from salience_detr_amd import synthetic as syn
    from salience_detr_amd.denoising import query_mask
    from salience_detr_amd.salience_decoder import SalienceTransformerDecoder, SalienceTransformerDecoderLayer
    if not torch.cuda.is_available():
        raise SystemExit("decoder_attention_train_micro: needs a HIP device (a time taken elsewhere says nothing)")
    dev = "cuda"
    layer = SalienceTransformerDecoderLayer(embed_dim=E, d_ffn=64, n_heads=H, dropout=0.0, n_levels=1, n_points=1)
    dec = SalienceTransformerDecoder(layer, 1, 3).to(dev).train()
    layer = dec.layers[0]
    result = {"bench": "decoder_attention_train_micro", "batch": B, "heads": H, "embed_dim": E, "iters": args.iters,
              "repeats": args.repeats, "unit": "us per forward + backward", "rows": {}}
    for N, (max_gt, groups) in CONFIGS.items():
        mask = query_mask(max_gt, groups, NQ).to(dev)
        assert tuple(mask.shape) == (N, N)
        q = syn.det_randn(f"atm.micro.q{N}", (B, N, E)).to(dev).requires_grad_(True)
        pos = syn.det_randn(f"atm.micro.pos{N}", (B, N, E)).to(dev).requires_grad_(True)
        w = syn.det_randn(f"atm.micro.w{N}", (B, N, E)).to(dev)

        def step(form):
            dec.set_train_form(form)
            layer._self_attention_train(q, pos, mask).backward(w)

        def window(form):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                step(form)
            stop.record()
            stop.synchronize()
            dec.zero_grad(set_to_none=True)
            q.grad = pos.grad = None
            return start.elapsed_time(stop) * 1000.0 / args.iters

        outs = {}
        for form in ("torch", "hip"):                      # results first: faster and different is not faster
            dec.set_train_form(form)
            outs[form] = layer._self_attention_train(q, pos, mask).detach()
        diff = (outs["hip"] - outs["torch"]).abs().max().item()
        for form in ("torch", "hip"):
            window(form)                                   # warm-up of every shape the timed windows use
        times = {"torch": [], "hip": []}
        for _ in range(args.repeats):
            for form in ("torch", "hip"):
                times[form].append(window(form))
        result["rows"][str(N)] = {
            form: {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
            for form, t in times.items()}
        result["rows"][str(N)]["max_abs_output_difference"] = diff
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
