"""tools/measure.py, the measuring harness of the tools/bench_<feature>.py scripts: what can be checked without a GPU -- the summary triple, the comparison's
wording and choice of base, the report lines, the child-process call, the report writing, the import rule, and that the scripts hold no copy of the method."""
import glob
import importlib.util
import json
import os
import py_compile
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
# the short GEMM and attention micro-benchmarks keep their own few lines of timing
OWN_TIMING = re.compile(r"bench_(gemm\w*|wgrad\w*|attn|adam|rowops|small_\w+|epilogue|grouped|cu_reserve|eval|decode_stress)\.py$")


def _load():
    spec = importlib.util.spec_from_file_location("measure", os.path.join(TOOLS, "measure.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


measure = _load()


def _runs(**medians):
    return {name.replace("_", " ").replace("parent ", "parent, "): [{"median_ms": m, "min_ms": m - 0.01, "max_ms": m + 0.01, "loss": 1.0} for m in ms] for name, ms in medians.items()}


def test_summary_odd_and_even():
    assert measure.summary([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert measure.summary([4.0, 1.0, 3.0, 2.0]) == (2.5, 1.0, 4.0)
    assert measure.summary([7.5]) == (7.5, 7.5, 7.5)


def test_verdict_wording_at_the_spread():
    inside = measure.verdict("text", "host rows", _runs(text=[10.29, 10.5], parent_host_rows=[10.0, 10.2]))
    assert inside == ["text against parent, host rows (best median of each): +2.90 %  -- no change in step time (inside the pool's box-to-box spread of +-3 %)"]
    slower = measure.verdict("text", "host rows", _runs(text=[10.31], parent_host_rows=[10.0]))
    assert slower == ["text against parent, host rows (best median of each): +3.10 %  -- SLOWER than the spread of +-3 %"]
    faster = measure.verdict("text", "host rows", _runs(text=[9.69], parent_host_rows=[10.0]))
    assert faster == ["text against parent, host rows (best median of each): -3.10 %  -- faster than the spread of +-3 %"]


def test_verdict_base_is_the_parent_when_it_was_run():
    runs = _runs(text=[10.0], host_rows=[5.0], parent_host_rows=[10.0])
    assert measure.verdict("text", "host rows", runs)[0].startswith("text against parent, host rows (best median of each): +0.00 %")
    del runs["parent, host rows"]
    lines = measure.verdict("text", "host rows", runs)
    assert lines[0].startswith("text against host rows (best median of each): +100.00 %  -- SLOWER") and lines[1:] == [measure.NO_PARENT]
    assert measure.NO_PARENT.startswith("(no --parent checkout given")
    # a script whose only in-tree variant is the new one compares against "parent" or not at all
    assert measure.verdict("unicode", None, _runs(unicode=[10.0])) == [measure.NO_PARENT]
    assert measure.verdict("unicode", None, _runs(unicode=[10.0], parent=[10.0]))[0].startswith("unicode against parent (best median of each): +0.00 %")


def test_step_lines_match_the_committed_report():
    with open(os.path.join(ROOT, "profiles", "phoc_bench.txt")) as f:
        committed = f.read().splitlines()
    runs = {"text": [{"median_ms": 5.866, "min_ms": 5.820, "max_ms": 5.956, "loss": 1820.915527}],
            "parent, host rows": [{"median_ms": 5.840, "min_ms": 5.785, "max_ms": 6.064, "loss": 1820.915894}]}
    lines = measure.step_lines(runs)
    assert lines == ["  text                    5.866 ms (5.820 .. 5.956)   loss 1820.915527", "  parent, host rows       5.840 ms (5.785 .. 6.064)   loss 1820.915894"]
    assert all(line in committed for line in lines)
    assert measure.step_lines({"text": runs["text"]}, tail=lambda r: "   metric %.6f" % 0.5)[0].endswith("loss 1820.915527   metric 0.500000")


def test_run_child_returns_the_last_line_and_puts_root_first(tmp_path):
    stub = tmp_path / "stub.py"
    stub.write_text("import json, os, sys\nprint('noise')\nprint(json.dumps({'argv': sys.argv[1:], 'path': os.environ['PYTHONPATH'].split(os.pathsep)[0], 'cwd': os.getcwd()}))\n")
    root = str(tmp_path)
    got = measure.run_child(str(stub), root, "batches.pt", "host rows", ["--graph"])
    assert got["argv"] == ["--child", "batches.pt", "--form", "host rows", "--root", root, "--graph"]
    assert got["path"] == root and os.path.realpath(got["cwd"]) == os.path.realpath(root)


def test_run_child_failure_carries_the_code_and_the_stderr_tail(tmp_path):
    stub = tmp_path / "stub.py"
    stub.write_text("import sys\nsys.stderr.write('x' * 3000 + ' the step was not captured')\nsys.exit(3)\n")
    with pytest.raises(SystemExit) as e:
        measure.run_child(str(stub), str(tmp_path), "batches.pt", "text")
    msg = str(e.value)
    assert "failed with 3" in msg and msg.endswith("the step was not captured") and len(msg) < 2200


def test_step_ab_alternates_the_variants(tmp_path, capsys):
    stub = tmp_path / "stub.py"
    stub.write_text("import json, sys, time\nprint(json.dumps({'form': sys.argv[4], 'extra': sys.argv[7:], 't': time.monotonic_ns(), 'median_ms': 1.5}))\n")
    root = str(tmp_path)
    runs = measure.step_ab(str(stub), [("a", root, "fa"), (("b", "captured"), root, "fb", ["--graph"])], "p", 2)
    assert [r["form"] for r in runs["a"]] == ["fa", "fa"] and [r["extra"] for r in runs[("b", "captured")]] == [["--graph"], ["--graph"]]
    order = sorted((r["t"], name) for name, rs in runs.items() for r in rs)
    assert [name for _, name in order] == ["a", ("b", "captured"), "a", ("b", "captured")]
    assert capsys.readouterr().err.splitlines() == ["a: 1.500 ms", "b, captured: 1.500 ms"] * 2          # one sign of life per child


def test_finish_writes_then_fails(tmp_path, capsys):
    out = tmp_path / "new" / "dir" / "report.txt"
    measure.finish(["one", "two"], str(out))
    assert out.read_text() == "one\ntwo\n" and capsys.readouterr().out == "one\ntwo\n"
    measure.finish(["printed only"], None)
    late = tmp_path / "late.txt"
    with pytest.raises(SystemExit) as e:
        measure.finish(["three"], str(late), ok=False, fail_msg="the kernel and the host twin disagree")
    assert str(e.value) == "the kernel and the host twin disagree" and late.read_text() == "three\n"


def test_arg_parser_flags():
    args = measure.arg_parser(parent=True, child=True).parse_args(["--child", "p", "--form", "text", "--out", "o"])
    assert (args.child, args.form, args.out, args.parent, args.root) == ("p", "text", "o", None, ROOT)
    assert measure.arg_parser(child=True, form="raw").parse_args(["--child", "p"]).form == "raw"
    with pytest.raises(SystemExit):
        measure.arg_parser().parse_args(["--parent", "x"])


def test_import_loads_neither_torch_nor_the_package():
    code = "import sys; sys.path.insert(0, %r); import measure; print(json.dumps([m in sys.modules for m in ('torch', 'numpy', 'sam_textvqa_amd')]))" % TOOLS
    r = subprocess.run([sys.executable, "-c", "import json; " + code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(TOOLS), timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    assert json.loads(r.stdout.decode()) == [False, False, False]


def test_every_bench_script_compiles(tmp_path):
    scripts = sorted(glob.glob(os.path.join(TOOLS, "bench_*.py")))
    assert len(scripts) >= 40
    for p in scripts + [os.path.join(TOOLS, "measure.py")]:
        py_compile.compile(p, cfile=str(tmp_path / (os.path.basename(p) + "c")), doraise=True)


def test_the_scripts_hold_no_copy_of_the_method():
    checked = [p for p in sorted(glob.glob(os.path.join(TOOLS, "bench_*.py"))) if not OWN_TIMING.search(p)]
    assert len(checked) >= 20
    for p in checked:
        with open(p) as f:
            text = f.read()
        for needle in ("def run_child", "def timed_alternating", "def window(", "torch.cuda.CUDAGraph()", "from tools.bench_aux_loss import"):
            assert needle not in text, "%s holds %r: the method lives in tools/measure.py" % (os.path.basename(p), needle)
