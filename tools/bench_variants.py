#!/usr/bin/env python3
"""Secondary measurements (not the driver's bench line): the TGLS (--gl-type GQ) and wLOD
(--weighted) variants of the path on a synthetic panel, one JSON line each.

    python tools/bench_variants.py [--snps 200000] [--inds 1000] [--winsize 100] [--steps 5]

--modes wlod_feed is a leg of its own: the weighted KDE feed (garlic_lod_feed, weighted, step = winsize) without and
with dictionary likelihoods, for every size of --winsizes on one resident panel; --tree DIR takes garlic_amd from another
checkout (the A/B against the parent commit: profiles/wlod_feed_ab.txt).  --modes tgls_feed: the same leg for the
unweighted feed with per-genotype likelihoods (use_gl, not weighted; --gl-kind codes or continuous; no LD weights), with the
kernel's fraction of the HBM roofline at the bytes per window of the form the call took (profiles/tgls_feed_ab.txt).
--modes tgls_slabs: garlic_lod_windows (device output) and garlic_roh_segments, and the weighted garlic_wlod_windows, sampled
feed (step = winsize) and garlic_roh_segments (weights: synthetic), with dictionary likelihoods under
GARLIC_GL_NO_TERMS=1 (the look-up chain), over the whole term matrix (first call and warm calls), and -- a library that has
garlic_panel_set_tgls_term_budget -- under every budget of --term-budgets-gb, with the device memory in use around the
calls (profiles/tgls_slabs_ab.txt; --tree for the parent commit).
--modes tgls_feed_multi: the TGLS KDE feeds of every size of --winsizes (step = size) on one resident panel with dictionary
likelihoods, as one garlic_lod_feed(use_gl) call per size and -- a library that has it -- as one garlic_lod_feed_multi_tgls
call, over the whole term matrix and under every budget of --term-budgets-gb: chain kernels, the whole call, chain launches,
term slabs built, device memory around the calls (--tree for the parent commit, which times the single calls only; set
GARLIC_TGLS_FEED_MULTI_SOLO=1 for the groups-of-one leg).
--modes ld_multi: the LD weights (no matrix output) of every size of --winsizes on one resident panel: a loop of single
garlic_panel_compute_ld calls and, where the library has it, one garlic_panel_compute_ld_multi call (--tree for the parent
commit, which times the loop only; several lists separated by ";" share one panel; profiles/ld_multi_ab.txt).
--modes feed_kde: the device KDE (garlic_lod_kde: moment and sums kernels by HIP events, the whole call) beside the sorted
garlic_lod_feed_subset call it replaces, at the --kde-inds and the everyone scale (--tree for the parent commit;
profiles/feed_kde_ab.txt).
--modes kde_multi: the KDEs of every size of --winsizes (step = size; a sweep: 50,100,200,300) on one resident panel, as a loop
of garlic_lod_kde per size (the path of the commits before garlic_lod_kde_multi, unchanged) beside one garlic_lod_kde_multi
call, at the --kde-inds and the everyone scale, with the moment and sums event times of both (profiles/kde_multi_ab.txt).
--modes feed_kde_parts: the KDE of a panel sharded over two panels on the one device: the present path (sorted feeds to the
host, merged, uploaded, garlic_feed_kde) beside garlic_lod_kde_part + garlic_kde_parts (profiles/kde_parts_ab.txt).
--modes kde_parts_multi: the KDEs of every size of --winsizes on a panel sharded over two panels on the one device: the loop of
garlic_lod_kde_part + garlic_kde_parts per size beside one garlic_lod_kde_part_set per shard + garlic_kde_parts_multi, at the
--kde-inds and the everyone scale; asserts that the structs agree bit for bit (profiles/kde_parts_multi_ab.txt).
--modes feature_counts: garlic_feature_counts at --snps hom rows x --inds individuals (the issue's shapes: 1000000 x 1250 and x
10000), 3 classes, 3 effects, hom-bit density 1e-3, 40 ROH per individual: the kernels by HIP events, the whole host-output
call, the bytes of row words and row fields one pass reads (profiles/feature_counts_ab.txt).
--modes feed_sort: the sorted KDE feed (garlic_panel_set_feed_order / garlic_feed_sort) on real thinned feeds of one
resident panel: the unweighted feed (step = winsize) of --kde-inds individuals (the --kde-subsample scale) and of
everyone -- the device sort alone by HIP events, its bytes per second at 24 B x keys x passes run, the whole feed call in
both orders, and on the same data one thread of std::sort and numpy's sort on the host, as stand-ins for gsl_sort
(profiles/feed_sort_ab.txt).
--modes bed_ingest: PLINK .bed input -- the census and the pack of a panel cut from a --file-inds file by HIP events with the bytes
each moves, and with --bed-prefix the whole garlic-lod run from .bed, TPED and genotype cache (--tree: the latter two with the
parent's tool); shapes 2M x 1280 and 10M x 1250 of a 10k-individual file; the table goes to profiles/bed_ingest_ab.txt.
--modes bed_extract: garlic_bed_extract of --inds individuals (1250) out of an image of --snps rows (1000000) x --file-inds
individuals (10000), scattered and contiguous, by HIP events: milliseconds and (source + written bytes) / time against the HBM
rate (profiles/bed_extract_ab.txt).
--modes feature_rows_bed: garlic_feature_set_rows_bed (hom rows from a .bed image of --snps rows x --file-inds individuals, every
row annotated and a sparse tenth) beside host-packed bit rows through garlic_feature_set_rows, both by HIP events, with the bytes
moved against the HBM peak (profiles/feature_rows_bed_ab.txt).
--modes ld_phased: the warm garlic_panel_compute_ld(phased = 1) call (weights only) for every size of --winsizes on one resident
panel -- host clock around the synchronous call and the ordered-sum kernel by the library's HIP events, median and spread
of --steps calls -- with the form the call took where the library reports it; and the phase upload from host memory both
ways, bytes and milliseconds: one byte per genotype (garlic_panel_set_phase) and bit rows (garlic_panel_set_phase_bits).
--modes tgls_dict16: GL-typed likelihoods with about 10,000 distinct values (three printed decimals after the clamp) on one
resident panel: through garlic_panel_set_gl_codes16 where the library has it (2 B per genotype), else through garlic_panel_set_gl
(continuous, 8 B per genotype: --tree for the parent commit).  The first TGLS score call (term pass + chain), warm calls (chain
alone), their difference as the term pass, the same after a change of frequencies (no re-upload with codes), and the device
memory in use (profiles/tgls_dict16_ab.txt).
--modes vcf_gl_parse: garlic_tgls_set_rows_vcf on device-resident VCF text of --snps lines x --inds samples beside
garlic_tgls_set_rows_text on the twin .tgls text of the same values, each call between stream events, GB/s of text
(profiles/vcf_gl_parse_ab.txt).
--tree for the parent commit; GARLIC_LD_PAIR_NO_MFMA=1 for this tree's AND + popcount form (profiles/ld_phased_mfma_ab.txt).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def wlod_feed_leg(args, tgls=False):
    """The whole garlic_lod_feed call (host clock around the synchronous call: scores, the two flatten passes, the feed's
    copy to the host buffer the call defines) and its score part / dominant kernel (the library's HIP events), repeated
    args.steps times after two warm-up calls; the score memory the call holds (garlic_device_alloc_stats, live + pooled)
    and the device memory in use after it.  score_part_ms is the library's total_ms: the MISSING fill and the score kernel;
    the flatten passes are part of call_ms only.  tgls: the unweighted feed with likelihoods instead of the weighted one
    (same panel, same fields, plus the score part's min / max and the kernel's roofline fraction)."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        if tgls and args.gl_kind == "continuous":      # real-valued GQ in [3, 60): more values than the dictionary holds
            gq = 3.0 + 57.0 * torch.rand(g.shape, generator=gen, device=dev, dtype=torch.float64)
        else:
            gq = torch.randint(3, 61, g.shape, generator=gen, device=dev).to(torch.float64)
        gl = torch.pow(torch.tensor(10.0, dtype=torch.float64, device=dev), -gq / 10.0)
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
        panel.set_gl_device(gl.data_ptr(), gl.shape[1], l0, gl.shape[0])
        del gq, gl
    del g
    full_bytes = int(panel.out_layout(32, nind)[2]) * 8
    for W in [int(w) for w in args.winsizes.split(",")]:
        if not tgls:
            ld = 1.0 + (max(2.0, W / 4.0) - 1.0) * torch.rand((nloci, W), generator=gen, device=dev, dtype=torch.float64)
            torch.cuda.synchronize()
            panel.set_ld_device(W, ld.data_ptr())
            del ld
        for step in [int(x) for x in args.feed_steps.split(",")] if args.feed_steps else [W]:
            for use_gl in ((True,) if tgls else (False, True)):
                panel.release_scratch()
                ctx.trim()
                torch.cuda.empty_cache()
                wall, score, kern = [], [], []
                for k in range(2 + args.steps):
                    t0 = time.perf_counter()
                    feed, _ = panel.lod_feed(W, error, max_gap, step, use_gl=use_gl, weighted=not tgls, copy=False)
                    dt = time.perf_counter() - t0
                    st = panel.stats()
                    if k >= 2:
                        wall.append(dt * 1e3)
                        score.append(st["total_ms"])
                        kern.append(st["chain_kernel_ms"])
                live, pooled, _ = ctx.alloc_stats()
                free_b, total_b = torch.cuda.mem_get_info()
                line = {"mode": "tgls_feed" if tgls else "wlod_feed", "snps": nloci, "inds": nind, "winsize": W, "step": step, "use_gl": use_gl,
                        "repeats": args.steps, "feed_values": int(feed.shape[0]),
                        "call_ms_median": float(np.median(wall)), "call_ms_min": min(wall), "call_ms_max": max(wall),
                        "score_part_ms_median": float(np.median(score)),
                        "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": min(kern), "kernel_ms_max": max(kern),
                        "score_memory_bytes": live + pooled, "full_score_matrix_bytes": full_bytes,
                        "device_memory_in_use_bytes": int(total_b - free_b),
                        "feed_checksum": float(np.sum(feed[np.isfinite(feed)]))}
                if hasattr(panel, "feed_info"):
                    line["feed_form"], line["score_doubles"] = panel.feed_info()
                if tgls:
                    # the ring chain's HBM bytes per window: terms in + the samples out (form 3; a library without
                    # garlic_lod_feed_info or with another form wrote full scores: 16.25 B)
                    line["gl_kind"] = args.gl_kind
                    line["score_part_ms_min"], line["score_part_ms_max"] = min(score), max(score)
                    per_win = 8.0 + 8.0 / step if line.get("feed_form") == 3 else 16.25
                    a = nloci * nind * per_win / (line["kernel_ms_median"] * 1e-3) / 1e9
                    line["roofline"] = {"bound": "hbm", "achieved": a, "peak": 8000.0, "unit": "GB/s", "frac": a / 8000.0,
                                        "algorithmic_bytes_per_window": per_win}
                print(json.dumps(line), flush=True)


def tgls_dict16_leg(args):
    """Wall clock around the synchronous garlic_lod_windows(use_gl, device output) call: the first call after an upload or a
    change of frequencies builds the terms and runs the chain, the following ones run the chain on resident terms (whole
    matrix) or build slabs again (--term-budget-gb); term_pass_ms is the median of the calls after a change of frequencies
    minus the median of the warm calls (under a budget every call builds its slabs, so it is near 0 there)."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    # GL column x = -k / 1000, k in [0, 10000): value 1 - 10^x, 0 -> 1e-16 (garlic-data.cpp:1557-1576)
    table = 1.0 - np.power(10.0, -np.arange(10000) / 1000.0)
    table[table <= 0] = 1e-16
    d_table = torch.from_numpy(table).to(dev)
    codes16 = hasattr(panel, "set_gl_codes16")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    t0 = time.perf_counter()
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        k = torch.randint(0, 10000, g.shape, generator=gen, device=dev)
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
        if codes16:
            panel.set_gl_codes16(k.to(torch.int32).cpu().numpy().astype(np.uint16), table, locus_begin=l0)
        else:
            gl = d_table[k]
            torch.cuda.synchronize()
            panel.set_gl_device(gl.data_ptr(), gl.shape[1], l0, gl.shape[0])
            del gl
        del k
    del g
    upload_s = time.perf_counter() - t0
    base, pitch, total = panel.out_layout(32, nind)
    out = torch.empty(total, dtype=torch.float64, device=dev)

    def call():
        torch.cuda.synchronize()
        t = time.perf_counter()
        panel.lod_windows_device(out.data_ptr(), W, error, max_gap, use_gl=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    if args.term_budget_gb:
        panel.set_tgls_term_budget(-1 if args.term_budget_gb < 0 else int(args.term_budget_gb * 1e9))
    # the very first call also carries the log10 probe, the table upload and the allocations: reported on its own
    first, warm, rebuild, reupload = call(), [], [], False
    for _ in range(args.steps):
        warm.append(call())
    try:
        for k in range(args.steps):          # new frequencies: the terms are built again
            panel.set_freq(np.clip(spec.freq * (1.0 + 1e-3 * (k + 1)), 0.0, 1.0))
            rebuild.append(call())
    except abi.GarlicError as e:
        reupload = str(e)
    free_b, total_b = torch.cuda.mem_get_info()
    line = {"mode": "tgls_dict16", "snps": nloci, "inds": nind, "winsize": W, "door": "set_gl_codes16" if codes16 else "set_gl",
            "tgls_mode": panel.tgls_mode()[0], "terms_by": panel.tgls_mode()[1], "upload_s": upload_s,
            "term_budget_gb": args.term_budget_gb,
            "first_call_ms": first, "rebuild_call_ms_median": float(np.median(rebuild)) if rebuild else None,
            "warm_call_ms_median": float(np.median(warm)), "warm_call_ms_min": min(warm), "warm_call_ms_max": max(warm),
            "term_pass_ms": float(np.median(rebuild)) - float(np.median(warm)) if rebuild else None, "chain_kernel_ms": panel.stats()["chain_kernel_ms"],
            "needs_reupload_after_set_freq": reupload, "device_memory_in_use_bytes": int(total_b - free_b),
            "likelihood_bytes": nloci * nind * (2 if codes16 else 8), "terms": nloci * nind,
            "checksum": float(out[base[0]: base[0] + nloci].nan_to_num(0.0, 0.0, 0.0).sum().item())}
    if hasattr(panel, "tgls_terms_info"):
        line["terms_info"] = panel.tgls_terms_info()
    print(json.dumps(line), flush=True)


def bed_extract_leg(args):
    """garlic_bed_extract on one device: an image of --snps rows x --file-inds individuals (random bytes made on the device),
    --inds of them extracted -- scattered over the whole file (random, ascending) and contiguous (a block in the middle).  The
    context runs on a torch stream, so torch's events (HIP events) bracket the call: the upload of the index list, the
    allocation of the new image, the kernel, the stream wait.  Per leg: milliseconds (median) and (source bytes + written
    bytes) / time against the HBM rate, for the source bytes the form must touch (the 16-byte pieces of the span's byte range
    per row, whole rows when the indices are spread over them) and for the whole source image."""
    import torch
    from garlic_amd import abi

    HBM_GBPS = 8000.0      # MI355X peak
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nrows, nfile, n_idx = args.snps, args.file_inds, args.inds
    rb = (nfile + 3) // 4
    stream = torch.cuda.Stream()
    ctx = abi.Context(0, stream=stream.cuda_stream)
    bed = abi.Bed(ctx, nrows, nfile)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    chunk = max(1, (256 << 20) // rb)
    for r in range(0, nrows, chunk):
        rows = torch.randint(0, 256, (min(chunk, nrows - r), rb), generator=g, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        bed.set_rows_device(rows.data_ptr(), rb, r, rows.shape[0])
    del rows
    rng = np.random.default_rng(7)
    start = (nfile - n_idx) // 2
    legs = {"scattered": np.sort(rng.choice(nfile, size=n_idx, replace=False)).astype(np.int32),
            "contiguous": np.arange(start, start + n_idx, dtype=np.int32)}
    for name, idx in legs.items():
        ms = []
        for k in range(1 + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sub = bed.extract(idx)
            e1.record(stream)
            torch.cuda.synchronize()
            sub.destroy()
            if k:
                ms.append(e0.elapsed_time(e1))
        t = float(np.median(ms))
        span = 8192      # subset individuals per workgroup: every span reads its own byte range of a row
        touched = sum(((int(idx[a:a + span].max()) >> 2) - (int(idx[a:a + span].min()) >> 2) + 16) for a in range(0, n_idx, span))
        written = nrows * ((n_idx + 3) // 4)
        line = {"mode": "bed_extract", "leg": name, "rows": nrows, "file_inds": nfile, "inds": n_idx, "repeats": args.steps,
                "call_ms_median": t, "source_bytes_touched": nrows * touched, "source_image_bytes": nrows * rb, "written_bytes": written,
                "touched_plus_written_GBps": (nrows * touched + written) / (t * 1e-3) / 1e9,
                "image_plus_written_GBps": (nrows * rb + written) / (t * 1e-3) / 1e9}
        line["fraction_of_HBM_peak_touched"] = line["touched_plus_written_GBps"] / HBM_GBPS
        print(json.dumps(line), flush=True)
    bed.destroy()
    ctx.close()


def feature_rows_bed_leg(args):
    """garlic_feature_set_rows_bed on one device beside the route it replaces, on the same data: an image of --snps rows x
    --file-inds individuals (random bytes made on the device) and two plans -- every image row annotated, and a sparse one of a
    tenth of the rows (sorted, random) -- selectors 0 / 1 at random.  The context runs on a torch stream, so torch's events (HIP
    events) bracket each call: for the new call the upload of the plan (9 bytes per row) and the kernel; for the baseline
    garlic_feature_set_rows of the same rows as host-packed bit rows (fetched once through garlic_feature_set_get_rows): the
    staged upload and the transpose kernel.  Per shape one JSON line: both medians, and the new call's bytes moved,
    rows x (ceil(nind / 4) + 8 ceil(nind / 64)), against the HBM peak."""
    import torch
    from garlic_amd import abi

    HBM_GBPS = 8000.0      # MI355X peak
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nimage, nind = args.snps, args.file_inds
    rb = (nind + 3) // 4
    stream = torch.cuda.Stream()
    ctx = abi.Context(0, stream=stream.cuda_stream)
    bed = abi.Bed(ctx, nimage, nind)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    chunk = max(1, (256 << 20) // rb)
    for r in range(0, nimage, chunk):
        rows = torch.randint(0, 256, (min(chunk, nimage - r), rb), generator=g, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        bed.set_rows_device(rows.data_ptr(), rb, r, rows.shape[0])
    del rows
    rng = np.random.default_rng(7)
    shapes = {"every_row": np.arange(nimage, dtype=np.int64),
              "sparse_tenth": np.sort(rng.choice(nimage, size=max(1, nimage // 10), replace=False)).astype(np.int64)}

    def timed(call, repeats):
        ms = []
        for k in range(1 + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    for name, file_row in shapes.items():
        n = int(file_row.shape[0])
        allele = rng.integers(0, 2, size=n).astype(np.uint8)
        with abi.FeatureSet(ctx, n, nind) as fs:
            t_bed = timed(lambda: fs.set_rows_bed(bed, file_row, allele), args.steps)
            host_rows = fs.get_rows()
            t_rows = timed(lambda: fs.set_rows(host_rows), max(1, min(args.steps, 2)))
            same = bool(np.array_equal(fs.get_rows(0, min(n, 4096)), host_rows[:4096]))
        moved = n * (rb + 8 * ((nind + 63) // 64))
        line = {"mode": "feature_rows_bed", "shape": name, "image_rows": nimage, "inds": nind, "rows": n, "repeats": args.steps,
                "rows_bed_ms_median": t_bed, "host_rows_ms_median": t_rows, "speedup": t_rows / t_bed if t_bed > 0 else None,
                "host_bytes_rows_bed": 9 * n, "host_bytes_host_rows": int(host_rows.nbytes), "bytes_moved": moved,
                "moved_GBps": moved / (t_bed * 1e-3) / 1e9, "fraction_of_HBM_peak": moved / (t_bed * 1e-3) / 1e9 / HBM_GBPS,
                "baseline_rows_read_back_equal": same}
        print(json.dumps(line), flush=True)
        del host_rows
    bed.destroy()
    ctx.close()


def bed_ingest_leg(args):
    """PLINK .bed input on one device.  The image's rows are random bytes made on the device (a file of --file-inds
    individuals, --snps rows); the context runs on a torch stream, so torch's events (HIP events) bracket the census call (the
    kernel and the read-back of 9 bytes per row) and the pack call (the upload of the per-word row list, 4 bytes per locus, and
    the kernel) of a panel of --inds individuals cut at --ind-offset.  With --bed-prefix P (P.bed / P.bim / P.fam, and the twins
    P.tped / P.tfam if present: garlic_amd.synth.write_bed_and_tped writes them) also the whole garlic-lod run -- load, census,
    upload, one feed -- from the .bed, from the TPED and from a genotype cache written by the first of them; --tree DIR runs
    the TPED and cache legs with another checkout's tool (the parent commit)."""
    import subprocess
    import tempfile
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, nfile = args.snps, args.inds, max(args.file_inds, args.inds + args.ind_offset)
    rb = (nfile + 3) // 4
    spec = synth.PanelSpec(nloci, seed=20260105)
    stream = torch.cuda.Stream()
    ctx = abi.Context(0, stream=stream.cuda_stream)
    bed = abi.Bed(ctx, nloci, nfile)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    chunk = max(1, (256 << 20) // rb)
    for r in range(0, nloci, chunk):
        rows = torch.randint(0, 256, (min(chunk, nloci - r), rb), generator=g, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        bed.set_rows_device(rows.data_ptr(), rb, r, rows.shape[0])
    first = rows[:1].clone()
    del rows
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    dest = np.arange(nloci, dtype=np.int64)

    def timed(fn):
        ms = []
        for k in range(1 + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def census():
        bed.set_rows_device(first.data_ptr(), rb, nloci - 1, 1)      # the same bytes again: the cached census is dropped
        bed.census()

    census_ms = timed(census)
    pack_ms = timed(lambda: panel.set_genotypes_bed(bed, dest, args.ind_offset))
    nblk = (nind + 126) // 64          # the panel's 64-individual blocks, its pad block included (nind_pad / 64): all are written
    line = {"mode": "bed_ingest", "snps": nloci, "inds": nind, "file_inds": nfile, "ind_offset": args.ind_offset,
            "repeats": args.steps, "census_call_ms_median_kernel_plus_9B_per_row_readback": census_ms, "census_image_bytes": nloci * rb,
            "census_GBps": nloci * rb / (census_ms * 1e-3) / 1e9, "pack_call_ms_median_row_list_upload_plus_kernel": pack_ms,
            "pack_genotype_bytes_of_the_column_block": nloci * ((nind + 3) // 4),
            "pack_bytes_fetched_upper_bound_with_16B_piece_overhead": nloci * ((nind + 3) // 4 + 31 * ((nblk + 63) // 64)),
            "pack_bytes_written_all_blocks": ((nloci + 15) // 16) * nblk * 256,
            "pack_row_list_bytes": 4 * nloci}
    panel.close()
    bed.destroy()
    if args.bed_prefix:
        P = args.bed_prefix
        tmp = tempfile.mkdtemp()
        cen = os.path.join(tmp, "centromeres.txt")
        with open(P + ".bim") as f, open(cen, "w") as c:
            for name in dict.fromkeys(l.split(None, 1)[0] for l in f):
                c.write("%s 0 0\n" % name)
        mine = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
        other = os.path.join(args.tree, "garlic_amd", "host", "garlic-lod") if args.tree else mine
        common = ["--centromere", cen, "--error", "0.001", "--winsize", str(args.winsize), "--kde-subsample", "0"]

        def wall(tool, inputs, tag):
            t0 = time.perf_counter()
            subprocess.check_call([tool, *inputs, "--out", os.path.join(tmp, tag), *common], stderr=subprocess.DEVNULL)
            return time.perf_counter() - t0

        line["tool_bfile_load_census_upload_one_feed_s"] = wall(mine, ["--bfile", P], "bed")
        if os.path.exists(P + ".tped"):
            cache = os.path.join(tmp, "twin.g2b")
            twin = ["--tped", P + ".tped", "--tfam", P + ".tfam"]
            line["tool_tped_load_upload_one_feed_s"] = wall(other, twin, "tped")
            line["tool_tped_load_cache_write_upload_one_feed_s"] = wall(other, twin + ["--genotype-cache", cache], "tpedc")
            line["tool_cache_load_upload_one_feed_s"] = wall(other, twin + ["--genotype-cache", cache], "cache")
            line["tped_and_cache_tool"] = other
    print(json.dumps(line), flush=True)


def feed_sort_leg(args):
    """The context runs on a torch stream, so torch's events (HIP events) bracket exactly the sort's kernels: the
    histogram, the plan and the passes that run (plus the 8-byte read-back of the pass count).  The feeds are the library's
    own: their top bytes repeat, so which passes drop out is the data's doing."""
    import ctypes
    import subprocess
    import tempfile
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    stream = torch.cuda.Stream()          # (not the null stream: the context would take a NULL handle for "create one")
    ctx = abi.Context(0, stream=stream.cuda_stream)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end)
    panel.set_freq(spec.freq)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
    del g
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, "libhost_sort.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "ubench", "host_sort.cpp")])
    host = ctypes.CDLL(so)
    host.host_std_sort_seconds.restype = ctypes.c_double
    host.host_std_sort_seconds.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    rng = np.random.default_rng(11)
    subsets = [np.sort(rng.choice(nind, size=min(args.kde_inds, nind), replace=False)).astype(np.int32), None]
    for idx in subsets:
        call = {}
        for order, name in ((abi.FEED_ORDER_REFERENCE, "reference"), (abi.FEED_ORDER_SORTED, "sorted")):
            panel.set_feed_order(order)
            wall = []
            for k in range(1 + args.steps):
                t0 = time.perf_counter()
                feed, _ = panel.lod_feed(W, error, max_gap, W, copy=False, ind_idx=idx)
                if k:
                    wall.append((time.perf_counter() - t0) * 1e3)
            call[name] = float(np.median(wall))
            if name == "reference":
                ref = feed.copy()
        n = int(ref.shape[0])
        assert np.array_equal(feed.view(np.uint64), np.sort(ref).view(np.uint64)), "sorted feed differs from numpy's sort"
        panel.set_feed_order(abi.FEED_ORDER_REFERENCE)
        d_ref = torch.from_numpy(ref).to(dev)
        ms = []
        for k in range(1 + args.steps):
            d = d_ref.clone()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.feed_sort(d.data_ptr(), n=n)
            e1.record(stream)
            torch.cuda.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        info = ctx.feed_sort_info()
        assert np.array_equal(d.cpu().numpy().view(np.uint64), feed.view(np.uint64))
        del d, d_ref
        x = ref.copy()
        std_s = host.host_std_sort_seconds(x.ctypes.data, n)
        x = ref.copy()
        t0 = time.perf_counter()
        x.sort()
        np_s = time.perf_counter() - t0
        sort_ms = float(np.median(ms))
        print(json.dumps({"mode": "feed_sort", "snps": nloci, "inds": nind, "winsize": W, "step": W,
                          "feed_individuals": nind if idx is None else int(idx.shape[0]), "keys": n, "repeats": args.steps,
                          "device_sort_ms_median": sort_ms, "device_sort_ms_min": min(ms), "device_sort_ms_max": max(ms),
                          "passes_run": info["passes_run"], "passes_skipped": info["passes_skipped"],
                          "sort_scratch_bytes": info["scratch_bytes"],
                          "traffic_GBps_at_24B_per_key_and_pass_run": 24.0 * n * info["passes_run"] / (sort_ms * 1e-3) / 1e9,
                          "feed_call_ms_reference_order": call["reference"], "feed_call_ms_sorted": call["sorted"],
                          "host_std_sort_1_thread_ms": std_s * 1e3, "host_numpy_sort_ms": np_s * 1e3,
                          "host_sorts_are": "stand-ins for gsl_sort (GSL is not available here); same data, this machine's host"}),
              flush=True)
        panel.release_scratch()


def feed_kde_leg(args):
    """The device KDE (garlic_lod_kde) beside the call it replaces, the sorted garlic_lod_feed_subset whose feed crosses to
    the host, on one resident panel, at the --kde-inds (--kde-subsample) and the everyone scale.  Per scale one JSON line:
    the host clock around the sorted feed call; where the library has garlic_lod_kde (--tree DIR for the parent commit,
    which has not: its line holds the feed call alone), the host clock and HIP events (the context runs on a torch stream)
    around the whole garlic_lod_kde call, and the library's own HIP-event times of the moment kernels (kde_moment_kernel
    + kde_tree_kernel, two passes) and the sums kernels (kde_sum_kernel + kde_slice_kernel): garlic_feed_kde_times."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    stream = torch.cuda.Stream()
    ctx = abi.Context(0, stream=stream.cuda_stream)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end)
    panel.set_freq(spec.freq)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
    del g
    have_kde = hasattr(panel, "lod_kde")
    rng = np.random.default_rng(11)
    subsets = [np.sort(rng.choice(nind, size=min(args.kde_inds, nind), replace=False)).astype(np.int32), None]
    for idx in subsets:
        panel.set_feed_order(abi.FEED_ORDER_SORTED)
        wall = []
        for k in range(1 + args.steps):
            t0 = time.perf_counter()
            feed, _ = panel.lod_feed(W, error, max_gap, W, copy=False, ind_idx=idx)
            if k:
                wall.append((time.perf_counter() - t0) * 1e3)
        n = int(feed.shape[0])
        line = {"mode": "feed_kde", "tree": os.path.abspath(args.tree) if args.tree else ROOT, "snps": nloci, "inds": nind,
                "winsize": W, "step": W, "feed_individuals": nind if idx is None else int(idx.shape[0]), "values": n,
                "feed_bytes_to_host": 8 * n, "repeats": args.steps, "sorted_feed_call_ms_median": float(np.median(wall)),
                "sorted_feed_call_ms_min": min(wall), "has_lod_kde": have_kde}
        panel.set_feed_order(abi.FEED_ORDER_REFERENCE)
        if have_kde:
            wall, ev, mom, sums = [], [], [], []
            for k in range(1 + args.steps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                kde, _ = panel.lod_kde(W, error, max_gap, W, ind_idx=idx)
                e1.record(stream)
                torch.cuda.synchronize()
                if k:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ev.append(e0.elapsed_time(e1))
                    t = ctx.feed_kde_times() if hasattr(ctx, "feed_kde_times") else {"moments_ms": float("nan"), "sums_ms": float("nan")}
                    mom.append(t["moments_ms"])
                    sums.append(t["sums_ms"])
            info = ctx.feed_kde_info()
            assert kde["n"] == n and kde["lo"] == feed[0] and kde["hi"] == feed[-1]
            line.update({"lod_kde_call_ms_median": float(np.median(wall)), "lod_kde_call_ms_min": min(wall),
                         "lod_kde_call_hip_events_ms_median": float(np.median(ev)),
                         "kde_moment_and_tree_kernels_ms_median": float(np.median(mom)),
                         "kde_sum_and_slice_kernels_ms_median": float(np.median(sums)),
                         "chunks": info["chunks"], "pairs_skipped": info["pairs_skipped"], "pairs": info["chunks"] * 512,
                         "kde_scratch_bytes": info["scratch_bytes"], "bandwidth": kde["h"],
                         "exp_per_s_of_pairs_not_skipped": (info["chunks"] * 512 - info["pairs_skipped"]) * 2048.0 / (float(np.median(sums)) * 1e-3)})
        print(json.dumps(line), flush=True)
        del feed
        panel.release_scratch()


def kde_multi_leg(args):
    """A window-size sweep's KDEs on one resident panel (unweighted --error scores, step = size): "loop" is one garlic_lod_kde
    per size, "multi" one garlic_lod_kde_multi over all sizes.  Per scale (--kde-inds individuals, everyone) one JSON line:
    the host clock around either (1 + --steps repeats, the first dropped; every repeat listed, so the spread shows), the
    sums of the loop's per-size moment and sums event times (garlic_feed_kde_times) and the multi call's own
    (garlic_feed_kde_multi_info), and whether the structs agree bit for bit."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    sizes = [int(w) for w in args.winsizes.split(",")]
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end)
    panel.set_freq(spec.freq)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
    del g
    rng = np.random.default_rng(11)
    subsets = [np.sort(rng.choice(nind, size=min(args.kde_inds, nind), replace=False)).astype(np.int32), None]
    for idx in subsets:
        loop_ms, loop_mom, loop_sums, multi_ms, multi_mom, multi_sums = [], [], [], [], [], []
        for k in range(1 + args.steps):          # the two paths in turn, so that a drift of the clocks meets both
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one, mom, sums = [], 0.0, 0.0
            for W in sizes:
                one.append(panel.lod_kde(W, error, max_gap, W, ind_idx=idx)[0])
                t = ctx.feed_kde_times()
                mom += t["moments_ms"]
                sums += t["sums_ms"]
            t1 = time.perf_counter()
            many, status, _ = panel.lod_kde_multi(sizes, error, max_gap, ind_idx=idx, strict=True)
            t2 = time.perf_counter()
            info = ctx.feed_kde_multi_info(len(sizes))
            if k:
                loop_ms.append((t1 - t0) * 1e3)
                multi_ms.append((t2 - t1) * 1e3)
                loop_mom.append(mom)
                loop_sums.append(sums)
                multi_mom.append(info["moments_ms"])
                multi_sums.append(info["sums_ms"])
        same = all(a["n"] == b["n"] and all(np.float64(a[f]).tobytes() == np.float64(b[f]).tobytes() for f in ("h", "sd", "q25", "q75", "lo", "hi"))
                   and all(a[f].tobytes() == b[f].tobytes() for f in ("x", "y", "raw")) for a, b in zip(one, many))
        print(json.dumps({"mode": "kde_multi", "snps": nloci, "inds": nind, "winsizes": sizes, "repeats": args.steps,
                          "feed_individuals": nind if idx is None else int(idx.shape[0]), "values": [int(k["n"]) for k in many],
                          "chunks": info["chunks"], "pairs_skipped": info["pairs_skipped"],
                          "loop_of_lod_kde_ms": loop_ms, "loop_of_lod_kde_ms_median": float(np.median(loop_ms)),
                          "lod_kde_multi_ms": multi_ms, "lod_kde_multi_ms_median": float(np.median(multi_ms)),
                          "loop_moment_kernels_ms_median": float(np.median(loop_mom)), "loop_sums_kernels_ms_median": float(np.median(loop_sums)),
                          "multi_moment_kernels_ms_median": float(np.median(multi_mom)), "multi_sums_kernels_ms_median": float(np.median(multi_sums)),
                          "multi_kernel_launches": info["kernel_launches"], "multi_host_waits": info["host_waits"],
                          "multi_scratch_bytes": info["scratch_bytes"], "structs_identical": bool(same)}), flush=True)
        panel.release_scratch()


def feed_kde_parts_leg(args):
    """The KDE of a panel sharded over two panels that split its individuals -- both on device 0, so this shows the saved
    transfer and host merge, NOT the scaling of the sums over devices.  Per scale (--kde-inds, everyone) one JSON line with
    two legs on real thinned feeds: "merged", the present several-shard path (every shard's sorted feed to the host, merged
    there -- numpy's sort of the concatenation stands in for the tool's merge --, uploaded, garlic_feed_kde), and "parts"
    (garlic_lod_kde_part per shard, garlic_kde_parts).  Host clock around each leg, warm-up call dropped, median and min;
    the library's HIP-event times of the sums kernels of either path."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    cut = nind // 2
    bounds = [(0, cut), (cut, nind)]
    ctxs = [abi.Context(0) for _ in bounds]
    panels = []
    for ctx, (b, e) in zip(ctxs, bounds):
        panel = abi.Panel(ctx, spec.chr_nloci, e - b)
        panel.set_map(spec.pos, spec.centro_start, spec.centro_end)
        panel.set_freq(spec.freq)
        panels.append(panel)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        for panel, (b, e) in zip(panels, bounds):
            half = g[:, b:e].contiguous()
            torch.cuda.synchronize()
            panel.set_genotypes_device(half.data_ptr(), half.shape[1], l0, half.shape[0])
            torch.cuda.synchronize()
    del g, half
    rng = np.random.default_rng(11)
    subsets = [np.sort(rng.choice(nind, size=min(args.kde_inds, nind), replace=False)).astype(np.int32), None]
    for idx in subsets:
        split = [None, None] if idx is None else [idx[idx < cut], idx[idx >= cut] - cut]
        legs = {}
        for leg in ("merged", "parts"):
            wall, sums_ms = [], []
            for k in range(1 + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg == "merged":
                    feeds = []
                    for panel, mine in zip(panels, split):
                        panel.set_feed_order(abi.FEED_ORDER_SORTED)
                        feeds.append(panel.lod_feed(W, error, max_gap, W, ind_idx=mine)[0])
                        panel.set_feed_order(abi.FEED_ORDER_REFERENCE)
                    t1 = time.perf_counter()
                    merged = np.sort(np.concatenate(feeds), kind="stable")
                    t2 = time.perf_counter()
                    kde = ctxs[0].feed_kde(merged)
                    dt = time.perf_counter() - t0
                    ms = [ctxs[0].feed_kde_times()["sums_ms"]]
                    extra = {"host_merge_ms": (t2 - t1) * 1e3, "feed_bytes_each_way": 8 * int(merged.shape[0])}
                else:
                    parts = [panel.lod_kde_part(W, error, max_gap, W, ind_idx=mine)[0] for panel, mine in zip(panels, split)]
                    kde = abi.kde_parts(parts)
                    dt = time.perf_counter() - t0
                    info = abi.kde_parts_info(parts)
                    ms = [float(v) for v in info["sums_ms"]]
                    extra = {"rank_rounds": info["rank_rounds"], "part_values": [p.count() for p in parts]}
                    for p in parts:
                        p.close()
                if k:
                    wall.append(dt * 1e3)
                    sums_ms.append(ms)
            legs[leg] = dict(extra, call_ms_median=float(np.median(wall)), call_ms_min=min(wall),
                             sums_kernels_ms_median=[float(v) for v in np.median(np.array(sums_ms), axis=0)],
                             n=int(kde["n"]), h=kde["h"], q25=kde["q25"], q75=kde["q75"])
        assert all(legs["merged"][k] == legs["parts"][k] for k in ("n", "q25", "q75")), legs
        print(json.dumps({"mode": "feed_kde_parts", "snps": nloci, "inds": nind, "winsize": W, "step": W, "shards": 2,
                          "devices": [0, 0], "feed_individuals": nind if idx is None else int(idx.shape[0]),
                          "repeats": args.steps, "merged": legs["merged"], "parts": legs["parts"]}), flush=True)
        for panel in panels:
            panel.release_scratch()


def kde_parts_multi_leg(args):
    """A window-size sweep's KDEs on a panel sharded over two panels that split its individuals, both on device 0 (so this
    shows launches, host waits and feed passes saved, NOT the scaling over devices; unweighted --error scores, step = size).
    "loop": per size garlic_lod_kde_part on either shard + garlic_kde_parts -- the path before garlic_kde_parts_multi,
    unchanged.  "sets": one garlic_lod_kde_part_set per shard + one garlic_kde_parts_multi.  Per scale (--kde-inds
    individuals, everyone) one JSON line: the host clock around either leg in turn (1 + --steps repeats, the first dropped;
    every repeat listed), the sets' launches, waits and event times (garlic_kde_parts_multi_info), and the assertion that
    the structs agree bit for bit."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    sizes = [int(w) for w in args.winsizes.split(",")]
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    cut = nind // 2
    bounds = [(0, cut), (cut, nind)]
    ctxs = [abi.Context(0) for _ in bounds]
    panels = []
    for ctx, (b, e) in zip(ctxs, bounds):
        panel = abi.Panel(ctx, spec.chr_nloci, e - b)
        panel.set_map(spec.pos, spec.centro_start, spec.centro_end)
        panel.set_freq(spec.freq)
        panels.append(panel)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        for panel, (b, e) in zip(panels, bounds):
            half = g[:, b:e].contiguous()
            torch.cuda.synchronize()
            panel.set_genotypes_device(half.data_ptr(), half.shape[1], l0, half.shape[0])
            torch.cuda.synchronize()
    del g, half
    rng = np.random.default_rng(11)
    subsets = [np.sort(rng.choice(nind, size=min(args.kde_inds, nind), replace=False)).astype(np.int32), None]
    for idx in subsets:
        split = [None, None] if idx is None else [idx[idx < cut], idx[idx >= cut] - cut]
        loop_ms, sets_ms, mom_ms, sums_ms = [], [], [], []
        for k in range(1 + args.steps):          # the two paths in turn, so that a drift of the clocks meets both
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one = []
            for W in sizes:
                parts = [panel.lod_kde_part(W, error, max_gap, W, ind_idx=mine)[0] for panel, mine in zip(panels, split)]
                one.append(abi.kde_parts(parts))
                for p in parts:
                    p.close()
            t1 = time.perf_counter()
            sets = [panel.lod_kde_part_set(sizes, error, max_gap, ind_idx=mine)[0] for panel, mine in zip(panels, split)]
            many, status = abi.kde_parts_multi(sets, strict=True)
            t2 = time.perf_counter()
            info = abi.kde_parts_multi_info(sets)
            part_values = [[int(v) for v in s.counts()] for s in sets]
            for s in sets:
                s.close()
            if k:
                loop_ms.append((t1 - t0) * 1e3)
                sets_ms.append((t2 - t1) * 1e3)
                mom_ms.append([float(v) for v in info["moments_ms"]])
                sums_ms.append([float(v) for v in info["sums_ms"]])
        same = all(a["n"] == b["n"] and all(np.float64(a[f]).tobytes() == np.float64(b[f]).tobytes() for f in ("h", "sd", "q25", "q75", "lo", "hi"))
                   and all(a[f].tobytes() == b[f].tobytes() for f in ("x", "y", "raw")) for a, b in zip(one, many))
        assert same, "garlic_kde_parts_multi differs from the loop of garlic_kde_parts"
        print(json.dumps({"mode": "kde_parts_multi", "snps": nloci, "inds": nind, "winsizes": sizes, "shards": 2, "devices": [0, 0],
                          "repeats": args.steps, "feed_individuals": nind if idx is None else int(idx.shape[0]),
                          "values": [int(k["n"]) for k in many], "part_values": part_values,
                          "loop_of_kde_parts_ms": loop_ms, "loop_of_kde_parts_ms_median": float(np.median(loop_ms)), "loop_of_kde_parts_ms_min": min(loop_ms),
                          "kde_parts_multi_ms": sets_ms, "kde_parts_multi_ms_median": float(np.median(sets_ms)), "kde_parts_multi_ms_min": min(sets_ms),
                          "set_moment_span_ms_median": [float(v) for v in np.median(np.array(mom_ms), axis=0)],
                          "set_sums_kernels_ms_median": [float(v) for v in np.median(np.array(sums_ms), axis=0)],
                          "set_kernel_launches": [int(v) for v in info["kernel_launches"]], "set_host_waits": [int(v) for v in info["host_waits"]],
                          "loop_host_waits_per_shard": 11 * len(sizes), "structs_identical": bool(same)}), flush=True)
        for panel in panels:
            panel.release_scratch()


def feature_counts_leg(args):
    """One JSON line.  The hom bits are drawn sparse (density x rows x individuals set bits at random places) and uploaded in
    slabs of rows; intervals: 40 per individual over 22 chromosomes, classes at random.  The count is checked against numpy on
    the first 64 individuals.  Host clock around the host-output call, warm-up call dropped; kernel_ms from the library."""
    import time
    from garlic_amd import abi

    nrows, nind, n_classes, n_effects, density, per_ind = args.snps, args.inds, 3, 3, 1e-3, 40
    rng = np.random.default_rng(20260301)
    chr_ = np.sort(rng.integers(0, 22, nrows)).astype(np.int32)
    pos = np.zeros(nrows, dtype=np.int32)
    for c in range(22):
        m = chr_ == c
        pos[m] = np.sort(rng.integers(1, 250000000, int(m.sum())))
    effect = rng.integers(0, n_effects, nrows).astype(np.int32)
    iv = np.zeros(nind * per_ind, dtype=abi.ROH_INTERVAL)
    iv["ind"] = np.repeat(np.arange(nind), per_ind)
    iv["chr"] = np.sort(rng.integers(0, 22, (nind, per_ind)), axis=1).reshape(-1)
    iv["start"] = rng.integers(1, 240000000, nind * per_ind)
    iv["stop"] = iv["start"] + rng.integers(100000, 5000000, nind * per_ind)
    iv["cls"] = rng.integers(0, n_classes, nind * per_ind)
    iv = iv[np.lexsort((iv["start"], iv["chr"], iv["ind"]))]
    same = (iv["ind"][1:] == iv["ind"][:-1]) & (iv["chr"][1:] == iv["chr"][:-1])      # an interval ends where the next begins, at the latest
    iv["stop"][:-1] = np.where(same, np.minimum(iv["stop"][:-1], iv["start"][1:]), iv["stop"][:-1])
    iv = np.ascontiguousarray(iv)
    row_bytes = (nind + 7) // 8
    first64 = np.zeros((nrows, 8), dtype=np.uint8)
    with abi.Context(0) as ctx, abi.FeatureSet(ctx, nrows, nind, chr=chr_, pos=pos, effect=effect) as fs:
        slab = max(1, (256 << 20) // row_bytes)
        for r0 in range(0, nrows, slab):
            n = min(slab, nrows - r0)
            bits = np.zeros((n, row_bytes), dtype=np.uint8)
            k = rng.binomial(n * nind, density)
            at_r, at_i = rng.integers(0, n, k), rng.integers(0, nind, k)
            np.bitwise_or.at(bits, (at_r, at_i >> 3), (1 << (at_i & 7)).astype(np.uint8))
            first64[r0:r0 + n, :min(8, row_bytes)] = bits[:, :8]
            fs.set_rows(bits, r0)
        wall, kern = [], []
        for k in range(1 + args.steps):
            t0 = time.perf_counter()
            counts = fs.counts(iv, n_classes, n_effects)
            dt = time.perf_counter() - t0
            info = fs.info()
            if k:
                wall.append(dt * 1e3)
                kern.append(info["kernel_ms"])
    # numpy on the first 64 individuals
    m = min(64, nind)
    hom = np.unpackbits(first64, axis=1, bitorder="little")[:, :m].astype(bool)
    key = chr_.astype(np.int64) * (1 << 32) + pos
    for i in range(m):
        rows = np.nonzero(hom[:, i])[0]
        mine = iv[iv["ind"] == i]
        starts = mine["chr"].astype(np.int64) * (1 << 32) + mine["start"]
        stops = mine["chr"].astype(np.int64) * (1 << 32) + mine["stop"]
        at = np.searchsorted(starts, key[rows], side="right") - 1
        inside = (at >= 0) & (key[rows] < stops[np.maximum(at, 0)])
        cls = np.where(inside, mine["cls"][np.maximum(at, 0)], n_classes)
        want = np.zeros((n_classes + 1, n_effects), dtype=np.int64)
        np.add.at(want, (cls, effect[rows]), 1)
        assert np.array_equal(counts[i], want), ("individual", i)
    nblk = (nind + 63) // 64
    words = nblk * nrows
    print(json.dumps({"mode": "feature_counts", "rows": nrows, "inds": nind, "classes": n_classes, "effects": n_effects, "density": density,
                      "intervals": int(iv.shape[0]), "blocks": info["blocks"], "chunks": info["chunks"], "words": words,
                      "words_skipped": info["words_skipped"], "row_word_bytes": 8 * words,
                      "row_field_bytes_at_most": 12 * (words - info["words_skipped"]),
                      "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": float(min(kern)),
                      "call_ms_median": float(np.median(wall)), "call_ms_min": float(min(wall)),
                      "row_words_GBps_at_median": 8 * words / (float(np.median(kern)) * 1e6) if np.median(kern) > 0 else None,
                      "counted": int(counts.sum()), "repeats": args.steps}), flush=True)


def tgls_slabs_leg(args):
    """Host clock around the synchronous calls (the term pass, where there is one, is part of the call).  One panel; legs in
    this order so that the code table (host work of the first use_gl call) is built before anything is timed as a first
    call: look-up chain, whole matrix, then the budgets."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        gq = torch.randint(3, 61, g.shape, generator=gen, device=dev).to(torch.float64)
        gl = torch.pow(torch.tensor(10.0, dtype=torch.float64, device=dev), -gq / 10.0)
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
        panel.set_gl_device(gl.data_ptr(), gl.shape[1], l0, gl.shape[0])
        del gq, gl
    del g
    total = panel.out_layout(32, nind)[2]
    out = torch.empty(total, dtype=torch.float64, device=dev)
    # the weighted legs: synthetic LD weights U(1, max(2, W/4)), an input of the calls timed here
    ld = 1.0 + (max(2.0, W / 4.0) - 1.0) * torch.rand((nloci, W), generator=gen, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    panel.set_ld_device(W, ld.data_ptr())
    del ld
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    wargs = dict(use_gl=True, weighted=True, M=7, mu=1e-9)

    def used():
        free_b, total_b = torch.cuda.mem_get_info()
        return int(total_b - free_b)

    def leg(name, budget_gb=None, weighted=True):
        line = {"mode": "tgls_slabs", "leg": name, "snps": nloci, "inds": nind, "winsize": W, "repeats": args.steps,
                "device_memory_before_bytes": used()}
        for what, call in (("windows", lambda: panel.lod_windows_device(out.data_ptr(), W, error, max_gap, use_gl=True)),
                           ("segments", lambda: panel.roh_segments(W, error, max_gap, args.cutoff, 0.25, use_gl=True)),
                           ("weighted_windows", lambda: panel.wlod_windows_device(out.data_ptr(), W, error, max_gap, 7, 1e-9, use_gl=True)),
                           ("weighted_feed", lambda: panel.lod_feed(W, error, max_gap, W, copy=False, **wargs)),
                           ("weighted_segments", lambda: panel.roh_segments(W, error, max_gap, args.cutoff, 0.25, **wargs))):
            if what.startswith("weighted") and not weighted:
                continue
            ms = []
            peak = used()
            for k in range(1 + args.steps):
                t0 = time.perf_counter()
                r = call()
                ms.append((time.perf_counter() - t0) * 1e3)
                peak = max(peak, used())
            line[what] = {"first_call_ms": ms[0], "warm_ms_median": float(np.median(ms[1:])), "warm_ms_min": min(ms[1:]),
                          "warm_ms_max": max(ms[1:]), "device_memory_peak_after_calls_bytes": peak}
            if what.endswith("segments"):
                line[what]["n_segments"] = len(r)
            if what == "weighted_feed":
                line[what]["feed_values"] = int(len(r[0]))
                line[what]["feed_form"] = panel.feed_info()[0]
            if hasattr(panel, "tgls_terms_info"):
                line[what].update(panel.tgls_terms_info())
            line[what]["device_memory_after_bytes"] = used()
        line["scores_checksum"] = float(out[: min(total, 1 << 24)].nan_to_num(0.0, 0.0, 0.0).sum().item())
        if budget_gb is not None:
            line["term_budget_gb"] = budget_gb
        print(json.dumps(line), flush=True)

    os.environ["GARLIC_GL_NO_TERMS"] = "1"
    leg("lookup chain (GARLIC_GL_NO_TERMS=1)", weighted=False)      # (the generic weighted kernel takes seconds per call)
    del os.environ["GARLIC_GL_NO_TERMS"]
    leg("whole matrix")
    if hasattr(panel, "set_tgls_term_budget"):
        for gb in [float(x) for x in args.term_budgets_gb.split(",") if x]:
            try:
                panel.set_tgls_term_budget(int(gb * 1e9))
            except abi.GarlicError as e:
                print(json.dumps({"mode": "tgls_slabs", "leg": "budget", "term_budget_gb": gb, "refused": str(e)}), flush=True)
                continue
            leg("budget", gb)


def tgls_feed_multi_leg(args):
    """Host clock around the synchronous calls; kernels: the library's events around the chain launches (a loop of single calls:
    the sum over its calls; under a budget the term passes run beside the chains and are inside neither kernel figure)."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    error, max_gap = 0.001, 200000
    sizes = [int(w) for w in args.winsizes.split(",")]
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        gq = torch.randint(3, 61, g.shape, generator=gen, device=dev).to(torch.float64)
        gl = torch.pow(torch.tensor(10.0, dtype=torch.float64, device=dev), -gq / 10.0)
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
        panel.set_gl_device(gl.data_ptr(), gl.shape[1], l0, gl.shape[0])
        del gq, gl
    del g
    torch.cuda.empty_cache()

    def used():
        free_b, total_b = torch.cuda.mem_get_info()
        return int(total_b - free_b)

    def singles():
        kern, total, n_slabs = 0.0, 0.0, 0
        for W in sizes:
            feed, _ = panel.lod_feed(W, error, max_gap, W, use_gl=True, copy=False)
            st = panel.stats()
            kern, total = kern + st["chain_kernel_ms"], total + float(np.sum(feed[np.isfinite(feed)]))
            if hasattr(panel, "tgls_terms_info"):
                n_slabs += panel.tgls_terms_info()["n_slabs"]
        return kern, total, {"n_chain_launches": max(n_slabs, len(sizes)), "n_term_builds": n_slabs}

    def multi():
        feeds, _ = panel.lod_feed_multi_tgls(sizes, max_gap, copy=False)
        info = panel.feed_multi_info(len(sizes))
        return panel.stats()["chain_kernel_ms"], float(sum(np.sum(f[np.isfinite(f)]) for f in feeds)), info

    def leg(name, call, budget_gb):
        line = {"mode": "tgls_feed_multi", "leg": name, "snps": nloci, "inds": nind, "winsizes": sizes, "repeats": args.steps,
                "solo_switch": bool(os.environ.get("GARLIC_TGLS_FEED_MULTI_SOLO")), "term_budget_gb": budget_gb,
                "device_memory_before_bytes": used()}
        wall, kern = [], []
        for k in range(2 + args.steps):
            t0 = time.perf_counter()
            k_ms, checksum, info = call()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                wall.append(dt)
                kern.append(k_ms)
        line.update({"call_ms_median": float(np.median(wall)), "call_ms_min": min(wall), "call_ms_max": max(wall),
                     "kernels_ms_median": float(np.median(kern)), "kernels_ms_min": min(kern), "kernels_ms_max": max(kern),
                     "feeds_checksum": checksum, "device_memory_after_bytes": used()})
        line.update(info)
        if hasattr(panel, "tgls_terms_info"):
            line.update(panel.tgls_terms_info())
        print(json.dumps(line), flush=True)

    budgets = [0.0] + ([float(x) for x in args.term_budgets_gb.split(",") if x] if hasattr(panel, "set_tgls_term_budget") else [])
    for gb in budgets:
        if gb:
            panel.set_tgls_term_budget(int(gb * 1e9))
        leg("single calls", singles, gb)
        if hasattr(panel, "lod_feed_multi_tgls"):
            leg("one multi call", multi, gb)


def ld_multi_leg(args):
    """Host clock around the synchronous calls, weights only (no LD matrix leaves the device); the device memory in use after
    each leg and, for the multi call, the bytes the installed sets hold and the passes it ran."""
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    size_lists = [[int(w) for w in part.split(",")] for part in args.winsizes.split(";")]      # several lists: one panel for all
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=200000)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
    del g
    torch.cuda.empty_cache()

    def used():
        free_b, total_b = torch.cuda.mem_get_info()
        return int(total_b - free_b)

    sizes = size_lists[0]

    def singles():
        for W in sizes:
            panel.compute_ld(W, want_output=False)
        return {}

    def multi():
        panel.compute_ld_multi(sizes, want_output=False)
        installed, groups, nbytes, n_pair, n_sum = panel.ld_info()
        return {"installed": installed, "groups": groups, "weight_bytes": nbytes, "n_pair_passes": n_pair, "n_sum_passes": n_sum}

    def leg(name, call):
        nonlocal sizes
        line = {"mode": "ld_multi", "leg": name, "snps": nloci, "inds": nind, "winsizes": sizes, "repeats": args.steps,
                "solo_switch": bool(os.environ.get("GARLIC_LD_MULTI_SOLO"))}
        wall = []
        for k in range(2 + args.steps):
            t0 = time.perf_counter()
            info = call()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                wall.append(dt)
        line.update({"call_ms_median": float(np.median(wall)), "call_ms_min": min(wall), "call_ms_max": max(wall),
                     "device_memory_after_bytes": used()})
        line.update(info)
        print(json.dumps(line), flush=True)

    for sizes_k in size_lists:
        sizes = sizes_k
        panel.release_scratch()
        leg("loop of single calls", singles)
        if hasattr(panel, "compute_ld_multi"):
            leg("one multi call", multi)


def ld_phased_leg(args):
    import time
    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind = args.snps, args.inds
    sizes = [int(w) for w in args.winsizes.split(",")]
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=200000)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
    del g
    torch.cuda.empty_cache()
    # the phase, slab by slab from host memory: bytes first, then (where the library has the call) the same values as bit rows,
    # which leaves the same planes
    rng = np.random.default_rng(11)
    slab = max(1, min(nloci, (1 << 30) // nind))
    up = {"bytes": [0, 0.0], "bits": [0, 0.0]}
    for l0 in range(0, nloci, slab):
        n = min(slab, nloci - l0)
        fc = rng.integers(0, 2, size=(n, nind), dtype=np.uint8)
        t0 = time.perf_counter()
        panel.set_phase(fc, locus_begin=l0)
        up["bytes"][1] += (time.perf_counter() - t0) * 1e3
        up["bytes"][0] += fc.nbytes
        if hasattr(panel, "set_phase_bits"):
            rows = np.packbits(fc, axis=1, bitorder="little")
            t0 = time.perf_counter()
            panel.set_phase_bits(rows, locus_begin=l0)
            up["bits"][1] += (time.perf_counter() - t0) * 1e3
            up["bits"][0] += rows.nbytes
    print(json.dumps({"mode": "ld_phased", "leg": "phase upload", "snps": nloci, "inds": nind,
                      "byte_upload_bytes": up["bytes"][0], "byte_upload_ms": up["bytes"][1],
                      "bit_upload_bytes": up["bits"][0], "bit_upload_ms": up["bits"][1]}), flush=True)
    for W in sizes:
        wall, kern = [], []
        for k in range(2 + args.steps):
            t0 = time.perf_counter()
            panel.compute_ld(W, want_output=False, phased=True)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                wall.append(dt)
                kern.append(ctx.recent_kernel_ms(1)[-1])
        line = {"mode": "ld_phased", "leg": "compute_ld", "snps": nloci, "inds": nind, "winsize": W, "repeats": args.steps,
                "no_mfma_switch": bool(os.environ.get("GARLIC_LD_PAIR_NO_MFMA")),
                "call_ms_median": float(np.median(wall)), "call_ms_min": min(wall), "call_ms_max": max(wall),
                "sum_kernel_ms_median": float(np.median(kern)), "sum_kernel_ms_min": min(kern), "sum_kernel_ms_max": max(kern)}
        if hasattr(panel, "ld_form_info"):
            pair, sumk, fused, phased = panel.ld_form_info()
            line.update({"pair_kernel": pair, "sum_kernel": sumk, "fused": fused})
        print(json.dumps(line), flush=True)
        panel.release_scratch()


def vcf_gl_parse_leg(args):
    """--modes vcf_gl_parse: garlic_tgls_set_rows_vcf on device-resident VCF text of --snps lines x --inds samples (e.g. 20000
    x 10000) beside garlic_tgls_set_rows_text on the twin .tgls text of the same GQ values, each call (parse,
    encode, status) between two events on the context's stream, in slabs of at most 256 MB of VCF text; GB/s of the text
    each reads.  Columns are `g|g:DP:GQ` with two-digit DP and GQ (10 bytes with the tab; the twin: 3 bytes)."""
    import torch
    from garlic_amd import abi

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nrows, nind = args.snps, args.inds
    stream = torch.cuda.Stream()
    ctx = abi.Context(0, stream=stream.cuda_stream)
    head_v = np.frombuffer(b"1\t1000000\trs0000000\tA\tG\t.\tPASS\t.\tGT:DP:GQ", dtype=np.uint8)
    head_t = np.frombuffer(b"1 rs0000000 0 1000000", dtype=np.uint8)
    slab_rows = max(1, min(nrows, (256 << 20) // (len(head_v) + 10 * nind + 1)))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def digits(v):      # two ASCII digits of every value
        return torch.stack([v // 10 + 48, v % 10 + 48], dim=-1).to(torch.uint8)

    def slab(n):
        gq = torch.randint(10, 100, (n, nind), generator=gen, device=dev)
        dp = torch.randint(10, 100, (n, nind), generator=gen, device=dev)
        gt = torch.randint(0, 2, (n, nind, 2), generator=gen, device=dev)
        v = torch.empty((n, len(head_v) + 10 * nind + 1), dtype=torch.uint8, device=dev)
        v[:, :len(head_v)] = torch.from_numpy(head_v.copy()).to(dev)
        cols = v[:, len(head_v):-1].view(n, nind, 10)
        cols[:, :, 0] = 9
        cols[:, :, 1] = (gt[:, :, 0] + 48).to(torch.uint8)
        cols[:, :, 2] = ord("|")
        cols[:, :, 3] = (gt[:, :, 1] + 48).to(torch.uint8)
        cols[:, :, 4] = ord(":")
        cols[:, :, 5:7] = digits(dp)
        cols[:, :, 7] = ord(":")
        cols[:, :, 8:10] = digits(gq)
        v[:, -1] = 10
        t = torch.empty((n, len(head_t) + 3 * nind + 1), dtype=torch.uint8, device=dev)
        t[:, :len(head_t)] = torch.from_numpy(head_t.copy()).to(dev)
        tc = t[:, len(head_t):-1].view(n, nind, 3)
        tc[:, :, 0] = 32
        tc[:, :, 1:3] = digits(gq)
        t[:, -1] = 10
        torch.cuda.synchronize()
        return v, t

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    ms = {"vcf": 0.0, "tgls": 0.0}
    nbytes = {"vcf": 0, "tgls": 0}
    with abi.Tgls(ctx, nrows, nind) as from_vcf, abi.Tgls(ctx, nrows, nind) as from_text:
        for step in range(args.steps + 1):          # the first round warms both kernels up and is not counted
            for r0 in range(0, nrows, slab_rows):
                n = min(slab_rows, nrows - r0)
                v, t = slab(n)
                lb_v = np.arange(n + 1, dtype=np.int64) * v.shape[1]
                lb_t = np.arange(n + 1, dtype=np.int64) * t.shape[1]
                dv = timed(lambda: from_vcf.set_rows_vcf(v.data_ptr(), lb_v, "GQ", row_begin=r0, text_bytes=v.numel(), where=abi.DEVICE))
                dt = timed(lambda: from_text.set_rows_text(t.data_ptr(), lb_t, row_begin=r0, text_bytes=t.numel(), where=abi.DEVICE))
                if step:
                    ms["vcf"] += dv
                    ms["tgls"] += dt
                    nbytes["vcf"] += v.numel()
                    nbytes["tgls"] += t.numel()
                if step == 0 and r0 == 0:
                    assert np.array_equal(from_vcf.get_rows(row_count=2), from_text.get_rows(row_count=2))
                del v, t
    print(json.dumps({"mode": "vcf_gl_parse", "lines": nrows, "samples": nind, "rounds": args.steps, "slab_lines": slab_rows,
                      "vcf_call_ms": ms["vcf"] / args.steps, "vcf_text_gb": nbytes["vcf"] / args.steps / 1e9,
                      "vcf_gb_per_s": nbytes["vcf"] / 1e6 / ms["vcf"],
                      "tgls_call_ms": ms["tgls"] / args.steps, "tgls_text_gb": nbytes["tgls"] / args.steps / 1e9,
                      "tgls_gb_per_s": nbytes["tgls"] / 1e6 / ms["tgls"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snps", type=int, default=200000)
    ap.add_argument("--inds", type=int, default=1000)
    ap.add_argument("--winsize", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--modes", default="lod,tgls,wlod")
    ap.add_argument("--winsizes", default="100,10", help="wlod_feed / tgls_feed: window sizes, one resident panel")
    ap.add_argument("--feed-steps", default="", help="wlod_feed / tgls_feed: thinning steps (default: the window size)")
    ap.add_argument("--gl-kind", default="codes", choices=["codes", "continuous"], help="tgls_feed: the likelihoods' form")
    ap.add_argument("--term-budgets-gb", default="8,12,32", help="tgls_slabs: garlic_panel_set_tgls_term_budget values to time")
    ap.add_argument("--term-budget-gb", type=float, default=0.0, help="tgls_dict16: garlic_panel_set_tgls_term_budget (GB; < 0: -1)")
    ap.add_argument("--cutoff", type=float, default=2.5, help="tgls_slabs: the LOD cutoff of the segments call")
    ap.add_argument("--kde-inds", type=int, default=20, help="feed_sort / feed_kde: individuals of the subsampled feed (--kde-subsample)")
    ap.add_argument("--file-inds", type=int, default=10000, help="bed_ingest: individuals of the .bed file the panel is cut from")
    ap.add_argument("--ind-offset", type=int, default=0, help="bed_ingest: the panel's first individual in the file")
    ap.add_argument("--bed-prefix", default="", help="bed_ingest: P.bed / P.bim / P.fam (and P.tped / P.tfam) for the whole-tool legs")
    ap.add_argument("--tree", default="", help="take garlic_amd from this checkout instead of the one the tool is in")
    args = ap.parse_args()
    if args.tree and args.modes != "bed_ingest":      # (bed_ingest: --tree names the tool of its TPED and cache legs only)
        sys.path.insert(0, os.path.abspath(args.tree))
    if args.modes == "tgls_slabs":
        return tgls_slabs_leg(args)
    if args.modes == "tgls_feed_multi":
        return tgls_feed_multi_leg(args)
    if args.modes == "ld_multi":
        return ld_multi_leg(args)
    if args.modes == "feed_sort":
        return feed_sort_leg(args)
    if args.modes == "feed_kde":
        return feed_kde_leg(args)
    if args.modes == "feature_counts":
        return feature_counts_leg(args)
    if args.modes == "feed_kde_parts":
        return feed_kde_parts_leg(args)
    if args.modes == "kde_multi":
        return kde_multi_leg(args)
    if args.modes == "kde_parts_multi":
        return kde_parts_multi_leg(args)
    if args.modes == "bed_extract":
        return bed_extract_leg(args)
    if args.modes == "bed_ingest":
        return bed_ingest_leg(args)
    if args.modes == "feature_rows_bed":
        return feature_rows_bed_leg(args)
    if args.modes == "ld_phased":
        return ld_phased_leg(args)
    if args.modes == "tgls_dict16":
        return tgls_dict16_leg(args)
    if args.modes == "vcf_gl_parse":
        return vcf_gl_parse_leg(args)
    if args.modes in ("wlod_feed", "tgls_feed"):
        return wlod_feed_leg(args, tgls=args.modes == "tgls_feed")

    import torch
    from garlic_amd import abi, synth

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nloci, nind, W = args.snps, args.inds, args.winsize
    error, max_gap = 0.001, 200000
    spec = synth.PanelSpec(nloci, seed=20260105, max_gap=max_gap)
    ctx = abi.Context(0)
    panel = abi.Panel(ctx, spec.chr_nloci, nind)
    panel.set_map(spec.pos, spec.centro_start, spec.centro_end, gpos=spec.gpos)
    panel.set_freq(spec.freq)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for l0, g in synth.genotype_chunks(spec, nind, dev):
        torch.cuda.synchronize()
        panel.set_genotypes_device(g.data_ptr(), g.shape[1], l0, g.shape[0])
        if "tgls" in args.modes or "wlodgl" in args.modes:
            # GQ ~ integer U{3..60}; error = 10^max(-10, -GQ/10)   (garlic-data.cpp:1557)
            gq = torch.randint(3, 61, g.shape, generator=gen, device=dev).to(torch.float64)
            gl = torch.pow(torch.tensor(10.0, dtype=torch.float64, device=dev), -gq / 10.0)
            torch.cuda.synchronize()
            panel.set_gl_device(gl.data_ptr(), gl.shape[1], l0, gl.shape[0])
            del gq, gl
    del g
    base, pitch, total = panel.out_layout(32, nind)
    out = torch.empty(total, dtype=torch.float64, device=dev)
    if "wlod" in args.modes:
        # synthetic LD weights U(1, W/4) until the LD kernel exists
        ld = 1.0 + (W / 4.0 - 1.0) * torch.rand((nloci, W), generator=gen, device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        panel.set_ld_device(W, ld.data_ptr())

    def run(mode):
        if mode == "lod":
            panel.lod_windows_device(out.data_ptr(), W, error, max_gap)
        elif mode == "tgls":
            panel.lod_windows_device(out.data_ptr(), W, error, max_gap, use_gl=True)
        elif mode == "wlodgl":
            panel.wlod_windows_device(out.data_ptr(), W, error, max_gap, 7, 1e-9, use_gl=True)
        else:
            panel.wlod_windows_device(out.data_ptr(), W, error, max_gap, 7, 1e-9)

    if "ld" in args.modes.split(","):
        # LD weights (calcHR2LD) from the resident genotypes, all individuals; wall clock of the call
        import time
        panel.compute_ld(W, want_output=False)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            panel.compute_ld(W, want_output=False)
        dt = (time.perf_counter() - t0) / args.steps
        print(json.dumps({"mode": "ld", "snps": nloci, "inds": nind, "winsize": W, "call_ms": dt * 1e3,
                          "loci_per_s": nloci / dt, "pair_counts_per_s": nloci * (W - 1) / dt,
                          "ld_sums_terms_per_s": nloci * W * W / dt}))
    if "feed" in args.modes.split(","):
        # KDE feed (garlic_lod_feed, unweighted, step = W): chain kernel with the thinned write-out, then
        # the compaction.  chain_kernel_ms = the chain kernel alone; call_ms = wall clock incl. the D2H
        # of the feed.
        import time
        panel.lod_feed(W, error, max_gap, W, copy=False)
        ms, wall = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            feed, _ = panel.lod_feed(W, error, max_gap, W, copy=False)
            wall.append(time.perf_counter() - t0)
            ms.append(panel.stats()["chain_kernel_ms"])
        k = float(np.mean(ms))
        print(json.dumps({"mode": "feed", "snps": nloci, "inds": nind, "winsize": W, "step": W,
                          "feed_values": int(feed.shape[0]), "chain_kernel_ms": k,
                          "call_ms": float(np.mean(wall)) * 1e3,
                          "sliding_windows_per_s": nloci * nind / (k * 1e-3),
                          }))
    for mode in [m for m in args.modes.split(",") if m not in ("ld", "feed")]:
        run(mode)
        ms = []
        for _ in range(args.steps):
            run(mode)
            ms.append(panel.stats()["chain_kernel_ms"])
        k = float(np.mean(ms))
        win = nloci * nind
        line = {"mode": mode, "snps": nloci, "inds": nind, "winsize": W, "kernel_ms": k,
                "sliding_windows_per_s": win / (k * 1e-3),
                "lod_windows_per_s": win / W / (k * 1e-3),
                "out_GBps": win * 8 / (k * 1e-3) / 1e9}
        # what bounds the kernel: HBM bytes per sliding window for the chains,
        # separately rounded FP64 multiply + add pairs for the weighted sums
        if mode in ("lod", "tgls"):
            per_win = 8.25 if mode == "lod" else 16.25
            a = win * per_win / (k * 1e-3) / 1e9
            line["roofline"] = {"bound": "hbm", "achieved": a, "peak": 8000.0, "unit": "GB/s", "frac": a / 8000.0,
                                "algorithmic_bytes_per_window": per_win}
        else:
            pairs = win * W / (k * 1e-3)
            line["roofline"] = {"bound": "fp64 valu (v_mul_f64 + v_add_f64 per term, no FMA)",
                                "achieved": 2 * pairs / 1e12, "peak": 78.6 / 2, "unit": "TFLOP/s",
                                "frac": 2 * pairs / 1e12 / (78.6 / 2),
                                "measured_ceiling_TFLOPs": 35.8, "frac_of_measured_ceiling": 2 * pairs / 1e12 / 35.8}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
