"""The programs plan_rtc.cpp generates, compiled without a GPU.

hipRTC compiles for gfx950 on any host, so tools/rtc_dump_local (built here
with the command its header comment gives) can generate and compile both
stages of every plan shape it knows.  A header edit that breaks only the
generated programs would otherwise go unseen: the engine falls back to the
interpreted kernel and the parity tests still pass.

Every program must also carry the shared device header (gg_pg_hash.h and
plan_dev.h, the text the host and plan.hip compile) exactly once, with
nothing but #define lines ahead of it.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TOOL_SRC = os.path.join(REPO, "tools", "rtc_dump_local.cpp")


def _tool_text():
    with open(TOOL_SRC) as f:
        return f.read()


def _shapes():
    """the shape names `rtc_dump_local ... all` runs"""
    m = re.search(r"const all\[\] = \{(.*?)\};", _tool_text(), re.S)
    return re.findall(r'"(\w+)"', m.group(1))


def _build_command():
    """the build line of the tool's header comment, as an argument list"""
    m = re.search(r"Build \(after the engine library\):\n(.*?)\n \* Usage",
                  _tool_text(), re.S)
    return re.sub(r"^ \*", "", m.group(1), flags=re.M).split()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if not shutil.which("hipcc") or not shutil.which("make"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", os.path.join(REPO, "greengage_amd", "csrc")],
                   check=True, capture_output=True)
    out = str(tmp_path_factory.mktemp("rtc") / "rtc_dump_local")
    cmd = [out if a == "tools/rtc_dump_local" else a.replace("$PWD", REPO)
           for a in _build_command()]
    assert out in cmd
    subprocess.run(cmd, check=True, cwd=REPO, capture_output=True)
    return out


@pytest.fixture(scope="module")
def shared_header():
    text = ""
    for path in ("include/gg_pg_hash.h", "greengage_amd/csrc/plan_dev.h"):
        with open(os.path.join(REPO, path)) as f:
            text += f.read()
    return text


def test_shape_list_is_the_documented_one():
    """every shape of `all` is described in the usage comment, so the
    parametrization below covers what the tool lists"""
    usage = _tool_text().split("Usage:")[1].split("*/")[0]
    listed = re.findall(r"^ \*   (\w+) ", usage, re.M)
    assert listed == _shapes() + ["all"]


@pytest.mark.parametrize("shape", _shapes())
def test_generated_programs_compile(tool, shared_header, tmp_path, shape):
    dump = str(tmp_path / "dump.cu")
    r = subprocess.run([tool, dump, shape], capture_output=True, text=True)
    # exit status 0 = every stage of the shape compiled under hipRTC
    assert r.returncode == 0, r.stderr
    with open(dump) as f:
        stages = re.split(r"/\* ==== nbake=\d+ ==== \*/\n", f.read())
    assert stages[0] == "" and len(stages) in (2, 3)
    for prog in stages[1:]:
        assert prog.count(shared_header) == 1
        ahead = prog[:prog.index(shared_header)]
        assert ahead and all(l.startswith("#define ")
                             for l in ahead.splitlines())
        assert "plan_kernel(PlanDev P)" in prog
