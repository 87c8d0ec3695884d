"""Event-timed cost of albedo demodulation (option svgf_demodulate) on the 1080p sponza stand-in, five a-trous levels.

  python tools/demod_times.py [--out profiles/demod_times.json] [--launches 40] [--warmup 10] [--rounds 3]

Medians over `launches` single launches (each between two events on the null stream, after `warmup` untimed ones), the arms alternated
round by round, option off and on in the same run and process:
  * temporal_{off,on}_us:    neb_svgf_temporal, the stand-alone same-pixel kernel ("svgf_fuse" = 0) / its demodulating arm;
  * last_level_{off,on}_us:  neb_svgf_atrous_level_rows of level 4 (step 16) over the whole frame / its remodulating arm;
  * chain_{off,on}_us:       neb_svgf_temporal + neb_svgf_atrous with "svgf_fuse" = 0 (the six separate kernels);
  * chain_fused_us:          neb_svgf_denoise with the option off: the default fused chain, which a context with the option on leaves.
A chain is one frame: neb_begin_frame (host only, outside the events) goes in front of each, the frame index counting up, so that the
demod plane is the valid history every time and the seed kernel never runs inside a timed chain (checked at the end through
"svgf_profile").  The repeated temporal calls stay in one bracket: the first seeds, the rest find the plane valid.
Both G-buffer slots hold the library's own G-buffer (neb_gbuffer_raycast) and 1-spp radiance.  Expected extra traffic: two albedo reads
(8 B/px) and one demod write (16 B/px) = 24 B/px = 50 MB at 1080p, against the chain's model of 82 + 46 L = 312 B/px.
Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import library_build_id
    from nebulae_amd import scene as S
    from nebulae_amd.renderer import DeferredRenderer, RenderInfo
    from nebulae_amd.svgf import PLANE_ALBEDO, PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE, SVGFDenoiser

    if not torch.cuda.is_available():
        raise SystemExit("demod_times: no GPU visible")
    W, H, L = 1920, 1080, 5
    r = DeferredRenderer()
    r.init(W, H, atrous_levels=L)
    r.begin_frame(RenderInfo(scene=S.atrium_standin(), camera=S.sponza_camera(), frame_index=1))
    r.submit_commands_gbuffer()
    r.submit_commands_pbr_lighting()
    r.submit_commands_gi_pathtrace()
    depth, normal, rad, albedo = (r.svgf.download(p) for p in (PLANE_DEPTH, PLANE_NORMAL, PLANE_RADIANCE, PLANE_ALBEDO))
    r.end_frame()
    r.destroy()

    frame = [2]

    def context(demod, fuse):
        d = SVGFDenoiser()
        d.init(W, H, atrous_levels=L)
        d.set_option("svgf_fuse", fuse)
        if demod:
            d.set_option("svgf_demodulate", 1)
        d.begin_frame(1)
        for slot in (0, 1):
            d.upload(PLANE_DEPTH, slot, depth)
            d.upload(PLANE_NORMAL, slot, normal)
            d.upload(PLANE_RADIANCE, slot, rad)
        d.upload(PLANE_ALBEDO, 0, albedo)
        return d

    off, on, fused = context(False, 0), context(True, 0), context(False, 1)

    def temporal(d):
        return None, lambda: d._check(d._lib.neb_svgf_temporal(d._ctx, None), "neb_svgf_temporal")

    def last_level(d):
        return None, lambda: d._check(d._lib.neb_svgf_atrous_level_rows(d._ctx, L - 1, 0, H, None), "neb_svgf_atrous_level_rows")

    def next_frame(d):
        def go():
            frame[0] += 1
            d.begin_frame(frame[0])
        return go

    def chain(d):
        def go():
            d._check(d._lib.neb_svgf_temporal(d._ctx, None), "neb_svgf_temporal")
            d._check(d._lib.neb_svgf_atrous(d._ctx, None), "neb_svgf_atrous")
        return next_frame(d), go

    def denoise(d):
        return next_frame(d), lambda: d._check(d._lib.neb_svgf_denoise(d._ctx, None), "neb_svgf_denoise")

    arms = {"temporal_off_us": temporal(off), "temporal_on_us": temporal(on), "last_level_off_us": last_level(off),
            "last_level_on_us": last_level(on), "chain_off_us": chain(off), "chain_on_us": chain(on), "chain_fused_us": denoise(fused)}
    samples = {k: [] for k in arms}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
    for _ in range(args.rounds):
        for name, (before, fn) in arms.items():
            for _ in range(args.warmup):
                if before:
                    before()
                fn()
            torch.cuda.synchronize()
            for a, b in ev:
                if before:
                    before()
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            samples[name] += [a.elapsed_time(b) * 1e3 for a, b in ev]
    res = {k: float(np.median(v)) for k, v in samples.items()}
    res.update({k.replace("_us", "_p10_p90_us"): [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for k, v in samples.items()})
    for k in ("temporal", "last_level", "chain"):
        res[f"{k}_extra_us"] = res[f"{k}_on_us"] - res[f"{k}_off_us"]
    res["chain_on_over_fused"] = res["chain_on_us"] / res["chain_fused_us"]
    res["chain_off_over_fused"] = res["chain_off_us"] / res["chain_fused_us"]
    # no seed kernel inside a chain of a running sequence
    on.set_option("svgf_profile", 1)
    before, go = chain(on)
    for _ in range(2):
        before()
        go()
    res["seed_launches_in_two_more_chains"] = int(on.level_times()[-1])
    px = W * H
    out = {"what": "svgf_demodulate cost, 1920x1080 sponza stand-in, L=5; medians of event-timed single launches (a chain = one frame)",
           "launches_per_arm": args.launches * args.rounds, "warmup": args.warmup, "build_id": library_build_id(),
           "device": torch.cuda.get_device_name(0), "expected_extra_bytes_per_pixel": 24, "expected_extra_mb": 24 * px / 1e6,
           "chain_model_bytes_per_pixel": 82 + 46 * L, **res}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for d in (off, on, fused):
        d.destroy()


if __name__ == "__main__":
    main()
