"""Every ``path/to/file.py:LINE`` citation of the reference (header, DESIGN.md, INTEGRATION.md, package and oracle
docstrings) points at a file that exists in the reference checkout and is at least that long.

The reference's file names and line counts are recorded in ``tests/golden/reference_files.json``, so the check runs
without the reference.  Where the reference checkout is mounted (``MMX_REFERENCE``), the record is compared with it as
well; ``python tests/test_citations.py --write`` rewrites the record from the checkout."""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MMX_REFERENCE", "/root/reference")
MANIFEST = os.path.join(ROOT, "tests", "golden", "reference_files.json")
EXTS = ("py", "rst", "yaml", "yml")
CITE = re.compile(r"((?:[A-Za-z_.][\w.-]*/)*[A-Za-z_][\w.-]*\.(?:py|rst|yaml|yml)):(\d+)")


def _scan(ref):
    """{path relative to the reference root: line count} of every citable file (glob semantics: hidden dirs skipped)."""
    out = {}
    for ext in EXTS:
        for path in glob.glob(os.path.join(ref, "**", "*." + ext), recursive=True):
            with open(path, errors="replace") as f:
                out[os.path.relpath(path, ref).replace(os.sep, "/")] = sum(1 for _ in f)
    return dict(sorted(out.items()))


def _load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def _resolve(rel, files):
    """Citations are written relative to the reference root, often with the leading directories elided ('.../x.py',
    bare 'lxmert_lrp.py').  Returns every reference file (a key of ``files``) the citation can mean."""
    if "/.../" in rel:                                              # 'lxmert/.../ExplanationGenerator.py'
        head, tail = rel.split("/.../", 1)
        head = head.strip("/")
        return [p for p in files if p.startswith(head + "/") and (p[len(head) + 1:] == tail or p.endswith("/" + tail))]
    rel = rel.lstrip("./")
    if rel in files:
        return [rel]
    return [p for p in files if p.endswith("/" + rel)]


def test_reference_citations_exist():
    files = _load_manifest()
    if os.path.isdir(REF):                                          # the record must still describe the reference
        assert _scan(REF) == files, "tests/golden/reference_files.json is stale: python tests/test_citations.py --write"
    sources = [os.path.join(ROOT, "include", "mmx_relevancy.h"), os.path.join(ROOT, "DESIGN.md"),
               os.path.join(ROOT, "INTEGRATION.md")]
    sources += glob.glob(os.path.join(ROOT, "transformer-mm-explainability_amd", "*.py"))
    sources += glob.glob(os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc", "*.h*"))
    sources += glob.glob(os.path.join(ROOT, "oracle", "*.py")) + glob.glob(os.path.join(ROOT, "oracle", "*.c"))
    bad, checked = [], 0
    for path in sources:
        text = open(path, errors="replace").read()
        for rel, line in CITE.findall(text):
            if rel.startswith(("transformer-mm-explainability_amd/", "tests/", "tools/", "oracle/", "profiles/", "examples/")):
                continue                                             # citations of this repository's own files
            if os.path.exists(os.path.join(ROOT, rel)) or os.path.exists(os.path.join(ROOT, "transformer-mm-explainability_amd", rel)) \
                    or os.path.exists(os.path.join(ROOT, "tests", rel)):
                continue                                             # one of this repository's own files
            targets = _resolve(rel, files)
            if not targets:
                bad.append("%s: %s:%s (no such reference file)" % (os.path.relpath(path, ROOT), rel, line))
                continue
            checked += 1
            if all(int(line) > files[t] for t in targets):
                bad.append("%s: %s:%s (file has %d lines)" % (os.path.relpath(path, ROOT), rel, line,
                                                              max(files[t] for t in targets)))
    assert checked > 100, "expected a few hundred resolvable citations, found %d" % checked
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_citations.py --write   (needs the reference checkout at $MMX_REFERENCE)")
    if not os.path.isdir(REF):
        raise SystemExit("no reference checkout at %s (set MMX_REFERENCE)" % REF)
    with open(MANIFEST, "w") as f:
        json.dump(_scan(REF), f, indent=0, sort_keys=True)
        f.write("\n")
