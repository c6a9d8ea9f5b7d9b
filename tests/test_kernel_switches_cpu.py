"""The kernel sources take exactly three build switches, the diagnostics builds: -DSVG_ABLATIONS (build.py --ablations; tools/pp_trace.py,
wg_timeline.py, vb_timeline.py), -DSVG_PROF_TRACE (tools/native_harness.hip) and -DSVG_KMEANS_TRACE (tools/native_svg2.hip).  A/B
switches of closed experiments do not stay in the sources: the value the product build uses is a plain constant, the measurement goes
into HISTORY.md / profiles/."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "sparse-videogen_amd" / "csrc"
DIAGNOSTICS = {"SVG_ABLATIONS", "SVG_PROF_TRACE", "SVG_KMEANS_TRACE"}
CONDITION = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif|elifdef|elifndef)\b(.*)$")


def switches():
    found = {}
    for src in sorted(CSRC.iterdir()):
        if src.suffix not in (".hip", ".h", ".inc"):
            continue
        for n, line in enumerate(src.read_text().splitlines(), 1):
            m = CONDITION.match(line)
            if m:
                for name in re.findall(r"\bSVG_\w+", m.group(2)):
                    found.setdefault(name, []).append(f"{src.name}:{n}")
    return found


def test_only_the_diagnostics_switches_remain():
    found = switches()
    extra = {k: v for k, v in found.items() if k not in DIAGNOSTICS}
    assert not extra, f"preprocessor switches beyond the diagnostics builds: {extra}"
    assert set(found) == DIAGNOSTICS, f"a diagnostics build lost its switch: {sorted(DIAGNOSTICS - set(found))}"
