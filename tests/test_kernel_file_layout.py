"""hk_kernels.hip is an include list (CPU, source text only): the device code lives in the stage headers, the file itself holds its
head comment, the system includes, `using namespace hkd;` and the includes, and the head comment is the index of those headers."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hikari.jl_amd", "csrc")


def _read():
    with open(os.path.join(CSRC, "hk_kernels.hip"), encoding="utf-8") as f:
        lines = f.read().split("\n")
    head = []   # the head comment: the `//` lines the file starts with
    for line in lines:
        if not line.startswith("//"):
            break
        head.append(line)
    code = "\n".join(re.sub(r"//.*", "", line) for line in lines)
    return "\n".join(head), code


def _stage_headers(code):
    return re.findall(r'^[ \t]*#[ \t]*include[ \t]+"(hk_\w+\.h)"', code, flags=re.M)


def test_kernel_file_holds_no_code():
    _, code = _read()
    for word in ("__global__", "HKD", "__device__", "#define"):
        assert word not in code, f"hk_kernels.hip holds `{word}`: device code belongs in the header of its stage"
    assert re.search(r"#\s*define", code) is None


def test_every_included_stage_header_exists():
    _, code = _read()
    headers = _stage_headers(code)
    assert len(headers) >= 12 and len(set(headers)) == len(headers)
    for h in headers:
        assert os.path.isfile(os.path.join(CSRC, h)), f"hk_kernels.hip includes {h}, which does not exist"


def test_head_comment_names_every_header_in_include_order():
    head, code = _read()
    at = -1
    for h in _stage_headers(code):
        found = re.search(r"(?<!\w)" + re.escape(h) + r"(?!\w)", head)
        assert found is not None, f"the head comment of hk_kernels.hip does not name {h}"
        assert found.start() > at, f"the head comment of hk_kernels.hip names {h} out of include order"
        at = found.start()
