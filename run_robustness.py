"""Fault-robustness sweep with the reference's interface (reference experiments/run_robustness.py).

    python run_robustness.py --data FOLDER|FILE.list [--error_space bitstream|latent]
        [--error_type random|burst|mask_replace|additive] [--rates 0,0.1,0.5,1,2,5,10] [--num_seeds 5]
        [--burst_len 8.0] [--sampler ddpm|ddim] [--steps 2] [--guidance_scale 1.0]
        [--output_csv indicators/robustness_results.csv] [--cache_dir encodings/] [--recon_dir outputs/robustness/]
        [--save_recon] [--force_encode] [--seed 231] [--suppress_warnings]
        [--ckpt FILE] [--dtype fp32|bf16] [--batch_size 8] [--lpips_backbone PATH [--lpips_lin PATH]]
        [--dists_weights PATH [--dists_backbone PATH]] [--thresholds_dir DIR] [--fec rs:NROOTS[:DEPTH]]

Per image: pad to x64 -> compress once to `<cache_dir>/<stem>` (kept: a later run decodes from that file and does not
encode again unless --force_encode) -> per (rate, seed) corrupt the stream (bitstream) or the decoded c_latent
(latent) -> decode -> crop -> score against the original (rdeic_amd/robustness.run_robustness). Writes --output_csv
with the columns image_id, error_space, error_type, error_rate (percent), seed, bpp, psnr, ssim, ms_ssim, lpips,
decode_failed, prints the per-rate mean / std table, and with --thresholds_dir writes
`<error_space>_<error_type>_failure_thresholds.csv` / `.txt` (reference experiments/plot_robustness.py:130-195).
Differences from the reference, all forced by the offline image or by design:
  * --ckpt / --dtype as inference.py (no checkpoint ships: the seeded synthetic weights stand in);
  * the variants of an image are entropy-decoded and relay-decoded in batches of --batch_size; a corrupted stream
    fails on its own (Compression.decompress(isolate=True)) and is the reference's failure row;
  * the clean latent is decoded from the cached stream, not from a cached `<stem>_latent.pt` (the stream is the record);
  * every metric runs on the device; lpips is NaN without --lpips_backbone; --dists_weights adds a `dists` column;
  * noise comes from one CPU generator per image seeded --seed (the reference draws on its CUDA generator);
  * --guidance_scale is accepted and, as in the reference (unconditional_conditioning=None), has no effect;
  * an --error_type that does not go with --error_space is refused at start-up (the reference runs `burst` then);
  * --fec (bitstream space only; refused at start-up with --error_space latent): the sweep the reference's study asks
    for and does not run. The Reed-Solomon protected stream (rdeic_amd/fec.py) is what gets corrupted, by the same
    corruptors and seeds; it is recovered, then decoded. A stream that does not recover is a failure row. bpp is the
    protected stream's rate, and the columns fec, bpp_payload, fec_corrected, fec_failed follow decode_failed. The
    cached `<cache_dir>/<stem>` stays the unprotected body. Without the flag every file, table and print is as before.
"""
import os
import sys
from argparse import ArgumentParser, Namespace
from typing import Dict, List

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None) -> Namespace:
    p = ArgumentParser(description="Run robustness experiments on the RDEIC codec")
    p.add_argument("--ckpt", default="", type=str, help="state dict (.pt/.ckpt, tensors only); empty = synthetic")
    p.add_argument("--config", default="", type=str, help="accepted for compatibility (architecture is fixed)")
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--data", type=str, required=True, help="path to an image folder or a .list file")
    p.add_argument("--error_space", type=str, choices=["bitstream", "latent"], default="bitstream",
                   help="where to inject errors")
    p.add_argument("--error_type", type=str, choices=["random", "burst", "mask_replace", "additive"],
                   default="random", help="type of error injection")
    p.add_argument("--rates", type=str, default="0,0.1,0.5,1,2,5,10", help="comma-separated error rates in percent")
    p.add_argument("--num_seeds", type=int, default=5, help="number of random seeds per rate")
    p.add_argument("--burst_len", type=float, default=8.0, help="mean burst length for burst errors")
    p.add_argument("--sampler", type=str, default="ddpm", choices=["ddpm", "ddim"])
    p.add_argument("--steps", type=int, default=2)
    p.add_argument("--guidance_scale", type=float, default=1.0)
    p.add_argument("--output_csv", type=str, default="indicators/robustness_results.csv")
    p.add_argument("--cache_dir", type=str, default="encodings/")
    p.add_argument("--recon_dir", type=str, default="outputs/robustness/")
    p.add_argument("--save_recon", action="store_true", help="save reconstructed images")
    p.add_argument("--force_encode", action="store_true", help="re-encode even if the cached stream exists")
    p.add_argument("--seed", type=int, default=231)
    p.add_argument("--device", type=str, default="cuda", choices=["cuda"])
    p.add_argument("--suppress_warnings", action="store_true")
    p.add_argument("--batch_size", type=int, default=8, help="variants of an image decoded together")
    p.add_argument("--lpips_backbone", type=str, default="",
                   help="torchvision AlexNet state dict (or the lpips package's); empty = lpips column NaN")
    p.add_argument("--lpips_lin", type=str, default="",
                   help="the LPIPS lin heads (.pth as the reference's, or .npz); default ./weight/lpips/alex.pth")
    p.add_argument("--dists_weights", type=str, default="",
                   help="DISTS alpha / beta (.pt / .pth / .npz); adds a dists column after lpips. Empty = no column")
    p.add_argument("--dists_backbone", type=str, default="",
                   help="torchvision VGG16 state dict for DISTS; empty = the convs are read from --dists_weights")
    p.add_argument("--thresholds_dir", type=str, default="",
                   help="write <error_space>_<error_type>_failure_thresholds.csv / .txt there")
    p.add_argument("--fec", type=str, default="",
                   help="rs:NROOTS[:DEPTH]: sweep the Reed-Solomon protected stream (bitstream space only)")
    args = p.parse_args(argv)
    args.fec_params = None
    if args.fec:
        from rdeic_amd.fec import parse_fec
        if args.error_space != "bitstream":
            p.error("--fec protects the bitstream: it does not go with --error_space latent")
        try:
            args.fec_params = parse_fec(args.fec)
        except ValueError as e:
            p.error(str(e))
    from rdeic_amd.robustness import check_error_pair
    try:
        check_error_pair(args.error_space, args.error_type)
    except ValueError as e:
        p.error(str(e))
    try:
        args.rate_list = [float(r) / 100.0 for r in args.rates.split(",") if r.strip()]
    except ValueError:
        p.error(f"--rates {args.rates!r} is not a comma-separated list of numbers")
    if not args.rate_list or any(r < 0 for r in args.rate_list):
        p.error("--rates needs at least one rate, none negative")
    if args.lpips_backbone and not args.lpips_lin:
        args.lpips_lin = os.path.join(".", "weight", "lpips", "alex.pth")
    if args.dists_backbone and not args.dists_weights:
        p.error("--dists_backbone needs --dists_weights")
    for what in ("lpips_backbone", "lpips_lin", "dists_weights", "dists_backbone"):  # refused at start-up
        path = getattr(args, what)
        if path and not os.path.isfile(path):
            p.error(f"--{what} {path} is not a file")
    if args.batch_size < 1 or args.num_seeds < 1 or args.steps < 1:
        p.error("--batch_size, --num_seeds and --steps must be >= 1")
    return args


def image_files(data: str) -> List[str]:
    """A .list file's lines, or every image under a folder (run_robustness.py:208-212)."""
    if os.path.isfile(data) and data.endswith(".list"):
        with open(data) as f:
            return [line.strip() for line in f if line.strip()]
    from inference import list_image_files
    return sorted(list_image_files(data))


def main(argv=None) -> List[Dict]:
    args = parse_args(argv)
    if args.suppress_warnings:
        import warnings
        warnings.filterwarnings("ignore")
    import numpy as np
    import torch
    from PIL import Image
    from inference import load_model
    from rdeic_amd import robustness as R
    from rdeic_amd.ood import pad64
    from rdeic_amd.synthetic import synth_context
    lpips_model = None
    if args.lpips_backbone:
        from rdeic_amd.lpips import LPIPS
        lpips_model = LPIPS("alex", backbone=args.lpips_backbone, lin=args.lpips_lin)
    dists_model = None
    if args.dists_weights:
        from rdeic_amd.dists import DISTS
        dists_model = DISTS(args.dists_weights, backbone=args.dists_backbone or None)
    model = load_model(args.ckpt, args.dtype)
    if model.cond_stage_model is not None:
        ctx = model.get_learned_conditioning([""])  # reference run_robustness.py:202
    else:
        ctx = synth_context().to(model.device)
    files = image_files(args.data)
    seeds = [args.seed + k for k in range(args.num_seeds)]
    print(f"Found {len(files)} images")
    print(f"Error rates: {[r * 100 for r in args.rate_list]}%")
    print(f"Error space: {args.error_space}, Error type: {args.error_type}")
    print(f"Seeds per rate: {args.num_seeds}")
    extra = {}
    if args.fec_params is not None:
        print(f"FEC: {args.fec_params.spec}")
        extra["fec"] = args.fec_params
    os.makedirs(args.cache_dir, exist_ok=True)

    groups: Dict = {}  # padded size -> files: one size after the other, so every launch plan is recorded once and reused
    for f in files:
        try:
            with Image.open(f) as im:
                w, h = im.size
            groups.setdefault((-(-h // 64) * 64, -(-w // 64) * 64), []).append(f)
        except Exception as e:  # noqa: BLE001
            print(f"Error processing {f}: {e}")

    def save_recon(rec: Dict, crop) -> None:
        d = os.path.join(args.recon_dir, rec["image_id"], f"r_{rec['error_rate']:.1f}", f"seed_{rec['seed']}")
        os.makedirs(d, exist_ok=True)
        Image.fromarray(crop).save(os.path.join(d, "recon.png"))

    done: Dict[str, List[Dict]] = {}
    encoded = cached = 0
    for key in sorted(groups):
        for f in groups[key]:
            stem = os.path.splitext(os.path.basename(f))[0]
            try:
                orig = np.array(Image.open(f).convert("RGB"))
                padded = torch.from_numpy(pad64(orig)[None]).to(model.device)
                stream_path = os.path.join(args.cache_dir, stem)
                if not os.path.exists(stream_path) or args.force_encode:
                    with open(stream_path, "wb") as fh:
                        fh.write(model.compress_images(padded)[0])
                    encoded += 1
                else:
                    cached += 1
                with open(stream_path, "rb") as fh:  # the sweep starts from the file (run_robustness.py:262-264)
                    body = fh.read()
                done[f] = R.run_robustness(
                    model, padded, ctx, args.error_space, args.error_type, args.rate_list, seeds, steps=args.steps,
                    sampler=args.sampler, noise_seed=args.seed, image_ids=[stem], mean_burst_len=args.burst_len,
                    batch_size=args.batch_size, lpips=lpips_model, dists=dists_model, orig_sizes=[orig.shape[:2]],
                    recon_cb=save_recon if args.save_recon else None, bodies=[body], **extra)
            except Exception as e:  # noqa: BLE001 — one unreadable image does not end the sweep
                print(f"Error processing {f}: {e}")
    print(f"Encoded {encoded} images, {cached} streams came from {args.cache_dir}")
    records = [r for f in files for r in done.get(f, [])]
    if not records:
        print("No results")
        return records
    R.write_records_csv(records, args.output_csv)
    print(f"\nResults saved to {args.output_csv}")
    print("\n=== Summary ===")
    print(R.format_summary(records))
    if args.thresholds_dir:
        R.write_failure_thresholds(records, args.thresholds_dir, prefix=f"{args.error_space}_{args.error_type}_")
        print(f"Failure thresholds saved to {args.thresholds_dir}")
    return records


if __name__ == "__main__":
    main()
