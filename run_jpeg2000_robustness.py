"""JPEG2000 robustness comparison with the reference's interface (reference experiments/run_jpeg2000_robustness.py).

    python run_jpeg2000_robustness.py --data FOLDER|FILE.list [--target_bpp 0.12] [--error_type random|burst]
        [--rates 0,0.1,0.5,1,2,5,10] [--num_seeds 5] [--burst_len 8.0] [--output_csv indicators/jpeg2000_robustness.csv]
        [--output_dir outputs/jpeg2000_robustness/] [--save_recon] [--seed 231]
        [--lpips_backbone PATH [--lpips_lin PATH]] [--dists_weights PATH [--dists_backbone PATH]]
        [--fec rs:NROOTS[:DEPTH]]

Every image is coded to JPEG2000 at about --target_bpp (the RDEIC stream's rate), the codestream gets the bit flips
the RDEIC sweep applies (run_robustness.py), and each decode is scored against the original: the columns codec,
image_id, error_type, error_rate (percent), seed, bpp, psnr, ssim, ms_ssim, lpips, decode_failed. Differences from
the reference (rdeic_amd/jpeg2000.py): the codec is Pillow's bundled OpenJPEG, not the opj_compress / opj_decompress
tools; a corrupted header that announces more than 4x the original's pixels is a failure row before any pixel is
decoded; the metrics run on the device (lpips NaN without --lpips_backbone; --dists_weights adds a `dists` column).
--fec (not in the reference) puts the codestream under the protection run_robustness.py --fec gives the RDEIC stream, so
that the two codecs are compared under the same code: the protected codestream is corrupted and recovered, one that
does not recover is a failure row, bpp is the protected rate, and fec, bpp_payload, fec_corrected, fec_failed follow
decode_failed.
"""
import os
import sys
from argparse import ArgumentParser, Namespace
from typing import Dict, List

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None) -> Namespace:
    p = ArgumentParser(description="Run JPEG2000 robustness experiments")
    p.add_argument("--data", type=str, required=True, help="path to an image folder or a .list file")
    p.add_argument("--target_bpp", type=float, default=0.12, help="target bits per pixel (match RDEIC's bpp)")
    p.add_argument("--error_type", type=str, choices=["random", "burst"], default="random",
                   help="type of error injection")
    p.add_argument("--rates", type=str, default="0,0.1,0.5,1,2,5,10", help="comma-separated error rates in percent")
    p.add_argument("--num_seeds", type=int, default=5, help="number of random seeds per rate")
    p.add_argument("--burst_len", type=float, default=8.0, help="mean burst length for burst errors")
    p.add_argument("--output_csv", type=str, default="indicators/jpeg2000_robustness.csv")
    p.add_argument("--output_dir", type=str, default="outputs/jpeg2000_robustness/")
    p.add_argument("--save_recon", action="store_true")
    p.add_argument("--seed", type=int, default=231)
    p.add_argument("--device", type=str, default="cuda", choices=["cuda"])
    p.add_argument("--lpips_backbone", type=str, default="",
                   help="torchvision AlexNet state dict (or the lpips package's); empty = lpips column NaN")
    p.add_argument("--lpips_lin", type=str, default="",
                   help="the LPIPS lin heads (.pth as the reference's, or .npz); default ./weight/lpips/alex.pth")
    p.add_argument("--dists_weights", type=str, default="",
                   help="DISTS alpha / beta (.pt / .pth / .npz); adds a dists column after lpips. Empty = no column")
    p.add_argument("--dists_backbone", type=str, default="",
                   help="torchvision VGG16 state dict for DISTS; empty = the convs are read from --dists_weights")
    p.add_argument("--fec", type=str, default="",
                   help="rs:NROOTS[:DEPTH]: sweep the Reed-Solomon protected codestream")
    args = p.parse_args(argv)
    args.fec_params = None
    if args.fec:
        from rdeic_amd.fec import parse_fec
        try:
            args.fec_params = parse_fec(args.fec)
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
    for what in ("lpips_backbone", "lpips_lin", "dists_weights", "dists_backbone"):
        path = getattr(args, what)
        if path and not os.path.isfile(path):
            p.error(f"--{what} {path} is not a file")
    if args.num_seeds < 1:
        p.error("--num_seeds must be >= 1")
    return args


def main(argv=None) -> List[Dict]:
    args = parse_args(argv)
    from rdeic_amd import jpeg2000 as J
    if not J.available():
        sys.exit("ERROR: this Pillow has no JPEG2000 codec (it was built without OpenJPEG); "
                 "the JPEG2000 baseline cannot run")
    import numpy as np
    import torch
    from PIL import Image
    from rdeic_amd import robustness as R
    from run_robustness import image_files
    lpips_model = None
    if args.lpips_backbone:
        from rdeic_amd.lpips import LPIPS
        lpips_model = LPIPS("alex", backbone=args.lpips_backbone, lin=args.lpips_lin)
    dists_model = None
    if args.dists_weights:
        from rdeic_amd.dists import DISTS
        dists_model = DISTS(args.dists_weights, backbone=args.dists_backbone or None)

    def score(pred, target) -> Dict:  # the project's device metrics on the whole (un-padded) image
        out = R.score_crop(torch.from_numpy(pred[None]).cuda(), torch.from_numpy(target[None]).cuda(), lpips_model,
                           dists_model)
        out["psnr"] = min(out["psnr"], 100.0)  # the reference's 1e-10 under the log caps a perfect match at 100 dB
        return out

    def save_recon(rec: Dict, pred) -> None:
        if rec["error_rate"] > 0:  # run_jpeg2000_robustness.py:229-232
            d = os.path.join(args.output_dir, rec["image_id"], f"r_{rec['error_rate']:.1f}")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(pred).save(os.path.join(d, f"seed_{rec['seed']}.png"))

    files = image_files(args.data)
    seeds = [args.seed + k for k in range(args.num_seeds)]
    print(f"Found {len(files)} images")
    print(f"Target BPP: {args.target_bpp}")
    print(f"Error rates: {[r * 100 for r in args.rate_list]}%")
    print(f"Error type: {args.error_type}")
    extra = {}
    if args.fec_params is not None:
        print(f"FEC: {args.fec_params.spec}")
        extra["fec"] = args.fec_params
    os.makedirs(args.output_dir, exist_ok=True)
    records: List[Dict] = []
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        try:
            img = np.array(Image.open(f).convert("RGB"))
            recs = J.run_jpeg2000_robustness([img], [stem], args.target_bpp, args.error_type, args.rate_list, seeds,
                                             args.burst_len, score=score,
                                             recon_cb=save_recon if args.save_recon else None, **extra)
            print(f"  {stem}: compressed at {recs[0]['bpp']:.4f} bpp")
            records += recs
        except Exception as e:  # noqa: BLE001
            print(f"Failed to compress {stem}: {e}")
    if not records:
        print("\nNo results to summarize - all compressions failed.")
        return records
    R.write_records_csv(records, args.output_csv, J.COLUMNS)
    print(f"\nResults saved to {args.output_csv}")
    print("\n=== Summary ===")
    print(R.format_summary(records))
    return records


if __name__ == "__main__":
    main()
