"""The measuring method of the tools/bench_<feature>.py scripts, in one place.  A script keeps its workloads, constants, report lines and twin-equality check;
how a number is taken is decided here.  Three timers, one question each:

  graph replay   replay_us (and its parts graph_of / timed_replays): the GPU time of a launch.  ROUNDS calls over distinct input sets are captured in one
                 graph and each replay is timed with one HIP event pair, so no host launch overhead is inside the pair; several forms take turns inside
                 each repetition.  Every form is warmed on every input set before its capture.
  eager window   window / timed_alternating (and peak for memory): what an eager caller pays -- host-issued calls with their launch gaps, allocator calls
                 and workspace queries -- in windows of `iters` calls between one event pair, the routes taking turns, the median window of each.
  fresh-process  step_child / run_child / step_ab / step_lines / verdict: the training step's time against the parent commit.  Every run is a fresh child
  A/B            process of the calling script that times `reps` steps one by one with an event pair each (the batch's clone outside the pair); the
                 variants alternate; the comparison takes the best median of each and reads it against SPREAD, the project's stated box-to-box spread.
  host_ms        wall time (time.perf_counter) of host work; a caller that times device work ends its function in a synchronise.

Every time is taken on the GPU or around work that ends in a synchronise: require_gpu fails where there is none, nothing falls back.  summary is the one
(median, min, max) that every script prints; arg_parser and finish are the scripts' shared command line and report writing.

Import rule.  A script imports this module from its own directory (`import measure`).  This module imports torch, numpy and sam_textvqa_amd inside its
functions only: a --child run with --root <built checkout of the parent commit> executes THIS tree's script and harness against the PARENT's package, so
the package must not be imported before the script has put --root on sys.path."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD = 0.03                                               # the box-to-box spread of the step time (README, DESIGN.md section 3.14 onward)
NO_PARENT = "(no --parent checkout given: the parent commit's step was not measured)"


def summary(values):
    """(median, min, max)"""
    v = sorted(values)
    n = len(v)
    return float(v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])), v[0], v[-1]


# ---- graph replay ----

def on_side_stream(body):
    """body() on a side stream that the current stream waits for: warm-up calls in front of a capture"""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


def graph_of(body):
    """(graph, body's return value) of one capture of body()"""
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = body()
    return g, out


def timed_replays(graphs, reps, per):
    """{name: summary of us per call}: `reps` replays of each graph of `per` calls, one event pair around each replay, the graphs taking turns inside
    each repetition"""
    import torch
    us = {name: [] for name in graphs}
    for _ in range(reps):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / per)
    return {name: summary(v) for name, v in us.items()}


def replay_us(forms, sets, rounds, reps):
    """forms: {name: fn(set)} in order, or one fn.  Every form is warmed on every set, captured as `rounds` calls over sets[i % len(sets)] and replayed
    once; then `reps` timed replays, the forms taking turns.  Returns ({name: summary of us per call}, {name: the last captured call's return value}), or
    the pair (summary, return value) for one fn."""
    import torch
    single = callable(forms)
    graphs, outs = {}, {}
    for name, fn in ({None: forms} if single else forms).items():
        for s in sets:
            fn(s)
        torch.cuda.synchronize()

        def body():
            for i in range(rounds):
                out = fn(sets[i % len(sets)])
            return out
        graphs[name], outs[name] = graph_of(body)
        graphs[name].replay()
    torch.cuda.synchronize()
    us = timed_replays(graphs, reps, rounds)
    return (us[None], outs[None]) if single else (us, outs)


# ---- eager windows ----

def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed_alternating(fns, iters, rounds=3, warm=5):
    """us per call of each fn: `rounds` windows of `iters` calls each, the routes taking turns; the median window of each"""
    import torch
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            got[k].append(window(fn, iters))
    return [sorted(g)[len(g) // 2] for g in got]


def peak(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def host_ms(fn, reps):
    """summary of the wall time of fn(r), r = 0 .. reps - 1, in ms"""
    ms = []
    for r in range(reps):
        t0 = time.perf_counter()
        fn(r)
        ms.append(1e3 * (time.perf_counter() - t0))
    return summary(ms)


# ---- fresh-process step A/B ----

def to_cuda(batch):
    import torch
    return {k: (v.cuda() if torch.is_tensor(v) else to_cuda(v) if isinstance(v, dict) else v) for k, v in batch.items()}


def step_child(path, form, make_step=None, *, use_graph, warm, reps, num_answers=5000, in_place=True, trainer_kw=None, extra=None):
    """The child's body: the c3 model's training step of the package importable from sys.path, on the batch `form` of the file; prints one JSON line.
    make_step(trainer, batch, form) returns the step to time (None: trainer.step).  Each of `reps` steps has its own event pair; its input is made outside
    the pair: a clone of the batch, or -- a captured step with in_place -- the graph's own input buffers.  extra(trainer): further keys of the line."""
    import torch
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.synthetic import clone_batch, mmt_config_dict, text_bert_config_dict
    from sam_textvqa_amd.trainer import Trainer
    batch = to_cuda(torch.load(path, weights_only=False)[form])
    torch.manual_seed(0)
    model = M.SAM4C(M.BertConfig.from_dict(mmt_config_dict(3)), M.BertConfig.from_dict(text_bert_config_dict()), num_answers=num_answers, bos_idx=1)
    trainer = Trainer(model, base_lr=1e-4, seed=1, use_graph=use_graph, **(trainer_kw or {}))
    step = make_step(trainer, batch, form) if make_step else trainer.step
    for _ in range(warm):
        step(clone_batch(batch))
    bufs = None
    if use_graph:
        assert trainer._graph is not None, "the step was not captured"
        bufs = trainer.input_buffers() if in_place else None
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        x = bufs if bufs is not None else clone_batch(batch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(x)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    m, a, z = summary(ms)
    print(json.dumps(dict({"form": form, "median_ms": m, "min_ms": a, "max_ms": z, "loss": float(loss)}, **(extra(trainer) if extra else {}))))


def run_child(script, root, path, form, extra=()):
    """one fresh process of `script` as --child against the package under `root`: its last output line, parsed"""
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(script), "--child", path, "--form", form, "--root", root] + list(extra), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, cwd=root)
    if r.returncode != 0:
        raise SystemExit("child (%s) failed with %d:\n%s" % (", ".join([root, form] + list(extra)), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def step_ab(script, variants, path, rounds):
    """variants: (name, root, form[, extra]) each.  {name: [run, ...]} of `rounds` children per variant, the variants alternating; one progress line per
    child on stderr."""
    runs = {v[0]: [] for v in variants}
    for _ in range(rounds):
        for name, root, form, *extra in variants:
            runs[name].append(run_child(script, root, path, form, *extra))
            print("%s: %.3f ms" % (name if isinstance(name, str) else ", ".join(name), runs[name][-1]["median_ms"]), file=sys.stderr, flush=True)
    return runs


def step_lines(runs, label_width=20, tail=None):
    """one report line per run; tail(run) adds a script's own columns"""
    return ["  %-*s %8.3f ms (%.3f .. %.3f)   loss %.6f%s" % (label_width, name, r["median_ms"], r["min_ms"], r["max_ms"], r["loss"], tail(r) if tail else "")
            for name, rs in runs.items() for r in rs]


def verdict(new, base, runs, spread=SPREAD):
    """The comparison lines: `new` against the parent's variant ("parent, <base>", or "parent" where base is None) when it was run, else against the
    in-tree `base` and a line that says the parent was not measured.  Best median of each; inside +-spread reads as no change."""
    parent = "parent, %s" % base if base else "parent"
    against = parent if parent in runs else base
    lines = []
    if against:
        best = lambda n: min(r["median_ms"] for r in runs[n])
        ratio = best(new) / best(against)
        pct = "+-%g %%" % (100 * spread)
        lines.append("%s against %s (best median of each): %+.2f %%  -- %s" % (new, against, 100 * (ratio - 1), "no change in step time (inside the pool's box-to-box spread of %s)" % pct
                                                                              if abs(ratio - 1) <= spread else "%s than the spread of %s" % ("SLOWER" if ratio > 1 else "faster", pct)))
    return lines + ([] if parent in runs else [NO_PARENT])


# ---- command line and report ----

def arg_parser(out=True, parent=False, child=False, form="text"):
    ap = argparse.ArgumentParser()
    if out:
        ap.add_argument("--out", default=None)
    if parent:
        ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    if child:
        ap.add_argument("--child", default=None)
        ap.add_argument("--form", default=form)
        ap.add_argument("--root", default=ROOT)
    return ap


def require_gpu(script_name):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s measures on the GPU; none found" % script_name)


def finish(lines, out, ok=True, fail_msg=None):
    """print the report, write it to `out` when given, and only then fail where the script's twin-equality check did"""
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit(fail_msg)
