"""Out-of-domain evaluation with the reference's interface (reference experiments/run_ood.py:279-441).

    python run_ood.py --domains ood/sketch,ood/xray [--sampler ddpm|ddim] [--steps 2] [--guidance_scale 1.0]
        [--latent_noise_std S --num_noise_samples N] [--output_dir indicators/] [--cache_dir encodings/ood/]
        [--save_recon] [--seed 231] [--ckpt FILE] [--dtype fp32|bf16] [--batch_size 1]
        [--lpips_backbone PATH [--lpips_lin PATH]] [--niqe_model FILE] [--brisque_model FILE]
        [--dists_weights PATH [--dists_backbone PATH]]
        [--fid_inception PATH [--fid_patch 256] [--kid_subset_size 1000]]

Per domain folder: pad to x64 -> compress to `<cache_dir>/<domain>/<stem>` -> decompress from that file -> relay
decode -> crop -> score against the original (rdeic_amd/ood.py). Writes `<output_dir>/ood_results_<domain>.csv` per
domain and `<output_dir>/ood_results_all.csv` with the columns domain, image_id, bpp, psnr, ssim, ms_ssim, lpips,
niqe, brisque, and prints the per-domain mean / std summary. --save_recon writes `<output_dir>/<domain>/<stem>.png`.
Differences from the reference, all forced by the offline image or by design:
  * --ckpt / --dtype as inference.py (no checkpoint ships: the seeded synthetic weights stand in);
  * every metric runs on the device; no metric weights ship with the project, so lpips is NaN without
    --lpips_backbone (AlexNet, as pyiqa "lpips"), niqe without --niqe_model (the published niqe_modelparameters.mat, or
    .npz / .safetensors with mu_prisparam, cov_prisparam) and brisque without --brisque_model (.npz / .safetensors
    with sv, sv_coef, rho, gamma, scale_min, scale_max);
  * --dists_weights PATH (alpha / beta; the VGG16 convs from --dists_backbone or from the same file) adds DISTS
    (rdeic_amd/dists.py) as a `dists` column after lpips; without the flag the tables are what they were. The
    best-of-N candidate is still chosen on LPIPS;
  * --fid_inception PATH (the InceptionV3 state dict, torchvision names) scores the sets, not the images: every
    reconstruction and its original go through the patch protocol (--fid_patch, 0 = whole images) and the feature
    tower (rdeic_amd/fid.py); `<output_dir>/fid_kid.csv` gets one row per domain and one row `all` (set, n_images,
    n_patches, fid, kid_mean, kid_std). The other tables do not change;
  * noise comes from a CPU generator seeded per image (--seed + the image's index in its domain's sorted order), so
    results do not depend on --batch_size.
"""
import os
import sys
from argparse import ArgumentParser, Namespace
from typing import Dict, List

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None) -> Namespace:
    p = ArgumentParser(description="Out-of-domain generalisation experiments on the RDEIC codec")
    p.add_argument("--ckpt", default="", type=str, help="state dict (.pt/.ckpt, tensors only); empty = synthetic")
    p.add_argument("--config", default="", type=str, help="accepted for compatibility (architecture is fixed)")
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--domains", type=str, required=True,
                   help="comma-separated list of domain folder paths (e.g. 'ood/sketch,ood/xray')")
    p.add_argument("--sampler", type=str, default="ddpm", choices=["ddpm", "ddim"])
    p.add_argument("--steps", type=int, default=2)
    p.add_argument("--guidance_scale", type=float, default=1.0)
    p.add_argument("--latent_noise_std", type=float, default=0.0,
                   help="standard deviation of the noise added to the latent (0 to disable)")
    p.add_argument("--num_noise_samples", type=int, default=1,
                   help="noisy candidates decoded per image; the lowest LPIPS against the padded original is kept")
    p.add_argument("--output_dir", type=str, default="indicators/")
    p.add_argument("--cache_dir", type=str, default="encodings/ood/")
    p.add_argument("--save_recon", action="store_true", help="save the reconstructed images")
    p.add_argument("--seed", type=int, default=231)
    p.add_argument("--device", type=str, default="cuda", choices=["cuda"])
    p.add_argument("--suppress_warnings", action="store_true")
    p.add_argument("--batch_size", type=int, default=1, help="images coded / decoded together (grouped by padded size)")
    p.add_argument("--lpips_backbone", type=str, default="",
                   help="torchvision AlexNet state dict (or the lpips package's); empty = lpips column NaN")
    p.add_argument("--lpips_lin", type=str, default="",
                   help="the LPIPS lin heads (.pth as the reference's, or .npz); default ./weight/lpips/alex.pth")
    p.add_argument("--niqe_model", type=str, default="",
                   help="niqe_modelparameters.mat (or .npz / .safetensors with mu_prisparam, cov_prisparam); "
                        "empty = niqe column NaN")
    p.add_argument("--brisque_model", type=str, default="",
                   help=".npz / .safetensors with sv, sv_coef, rho, gamma, scale_min, scale_max; "
                        "empty = brisque column NaN")
    p.add_argument("--dists_weights", type=str, default="",
                   help="DISTS alpha / beta (.pt / .pth / .npz); adds a dists column after lpips. Empty = no column")
    p.add_argument("--dists_backbone", type=str, default="",
                   help="torchvision VGG16 state dict (or the lpips package's) for DISTS; empty = the convs are "
                        "read from --dists_weights (stage<k>.<i>.*)")
    from rdeic_amd import fid as _fid
    _fid.add_cli_flags(p)
    args = p.parse_args(argv)
    _fid.check_cli_flags(p, args)
    if args.lpips_backbone and not args.lpips_lin:
        args.lpips_lin = os.path.join(".", "weight", "lpips", "alex.pth")
    if args.dists_backbone and not args.dists_weights:
        p.error("--dists_backbone needs --dists_weights")
    for what in ("lpips_backbone", "lpips_lin", "niqe_model", "brisque_model", "dists_weights",
                 "dists_backbone"):  # refused at start-up
        path = getattr(args, what)
        if path and not os.path.isfile(path):
            p.error(f"--{what} {path} is not a file")
    if args.batch_size < 1 or args.num_noise_samples < 1 or args.latent_noise_std < 0:
        p.error("--batch_size and --num_noise_samples must be >= 1 and --latent_noise_std >= 0")
    return args


def print_summary(records: List[Dict], with_dists: bool = False) -> None:
    from rdeic_amd.ood import columns, summary
    print("\n=== Overall Summary by Domain (mean, std) ===")
    for domain, cols in summary(records, with_dists).items():
        print(f"{domain}: " + ", ".join(f"{k} {cols[k][0]:.4f} ({cols[k][1]:.4f})" for k in columns(with_dists)[2:]))


def main(argv=None) -> List[Dict]:
    args = parse_args(argv)
    if args.suppress_warnings:
        import warnings
        warnings.filterwarnings("ignore")
    from inference import list_image_files, load_model
    from rdeic_amd import metrics, ood
    from rdeic_amd.synthetic import synth_context
    lpips_model = None
    if args.lpips_backbone:
        from rdeic_amd.lpips import LPIPS
        lpips_model = LPIPS("alex", backbone=args.lpips_backbone, lin=args.lpips_lin)
    dists_model = None
    if args.dists_weights:
        from rdeic_amd.dists import DISTS
        dists_model = DISTS(args.dists_weights, backbone=args.dists_backbone or None)
    fid_tower, fid_rows, fid_all = None, [], None
    if args.fid_inception:
        from rdeic_amd import fid as _fid
        fid_tower = _fid.InceptionV3(args.fid_inception)
        fid_all = _fid.FidKid(fid_tower, args.fid_patch)
    niqe_model = metrics.NIQE(args.niqe_model) if args.niqe_model else None
    brisque_model = metrics.BRISQUE(args.brisque_model) if args.brisque_model else None
    model = load_model(args.ckpt, args.dtype)
    if model.cond_stage_model is not None:
        ctx = model.get_learned_conditioning([""])  # reference run_ood.py:292
    else:
        ctx = synth_context().to(model.device)
    print(f"sampling {args.steps} steps using {args.sampler} sampler")
    all_records: List[Dict] = []
    for domain_path in [d.strip() for d in args.domains.split(",") if d.strip()]:
        name = os.path.basename(os.path.normpath(domain_path))
        print(f"\nProcessing domain: {name}")
        if not os.path.isdir(domain_path):
            print(f"Warning: {domain_path} is not a directory, skipping")
            continue
        files = list_image_files(domain_path)
        print(f"Found {len(files)} images")
        fid_run = _fid.FidKid(fid_tower, args.fid_patch) if fid_tower is not None else None
        records = ood.run_domain(
            model, files, ctx, domain=name, cache_dir=args.cache_dir, sampler=args.sampler, steps=args.steps,
            guidance_scale=args.guidance_scale, latent_noise_std=args.latent_noise_std,
            num_noise_samples=args.num_noise_samples, seed=args.seed, batch_size=args.batch_size, lpips=lpips_model,
            niqe_model=niqe_model, brisque_model=brisque_model,
            recon_dir=os.path.join(args.output_dir, name) if args.save_recon else None, dists=dists_model,
            fid=fid_run)
        if fid_run is not None:
            fid_all.merge(fid_run)
            if fid_run.n_patches >= 2:  # a domain with fewer patches has no covariance: it counts in `all` only
                fid_rows.append({"set": name, **fid_run.result(kid_subset_size=args.kid_subset_size)})
                print(f"{name}: " + _fid.summary_line(fid_rows[-1]))
        if records:
            path = os.path.join(args.output_dir, f"ood_results_{name}.csv")
            ood.write_csv(records, path, dists_model is not None)
            print(f"Domain results saved to {path}")
            all_records += records
    if all_records:
        path = os.path.join(args.output_dir, "ood_results_all.csv")
        ood.write_csv(all_records, path, dists_model is not None)
        print(f"\nConsolidated results saved to {path}")
        print_summary(all_records, dists_model is not None)
    if fid_all is not None and fid_all.n_patches < 2:
        print(f"FID / KID need at least 2 patches on each side, got {fid_all.n_patches}: fid_kid.csv not written")
    elif fid_all is not None:
        fid_rows.append({"set": "all", **fid_all.result(kid_subset_size=args.kid_subset_size)})
        print(_fid.summary_line(fid_rows[-1]))
        _fid.write_csv(fid_rows, os.path.join(args.output_dir, "fid_kid.csv"))
    return all_records


if __name__ == "__main__":
    main()
