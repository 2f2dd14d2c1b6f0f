"""Generates tests/golden/script_templates.json: every `cat > file.cfg <<EOF ... EOF` configuration template of the
reference's pipeline scripts (test/*.sh), with the shell variables replaced by a fixed token, together with what the
SHA-256 of what the REFERENCE's own parser (oracle/_ref/libreadconfig_ref.so, built by oracle/Makefile) says of each,
read as a file and through a command line (the canonical JSON of tests/test_config.py: canon(scrub(dump))).  Run from the repo root with the reference's test directory as the argument:
    python tests/golden/make_script_templates_golden.py REFERENCE/test"""
import glob
import hashlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ref_readconfig as rr    # noqa: E402

ARGV = ["tool", "averaging_method=total-transmission", "@path", "output=out.h5"]


def script_templates(test_dir):
    """(script, target, text) for every here-document that writes a .cfg file."""
    out = []
    for path in sorted(glob.glob(os.path.join(test_dir, "*.sh"))):
        src = open(path, errors="replace").read()
        for m in re.finditer(r"cat\s*>\s*(\S+)\s*<<\s*EOF\n(.*?)\nEOF", src, re.S):
            text = re.sub(r"\$\{[^}]*\}|\$[A-Za-z_][A-Za-z_0-9]*", "VAR", m.group(2)) + "\n"
            out.append((os.path.basename(path), m.group(1), text))
    return out


def scrub(obj, d):
    return json.loads(json.dumps(obj).replace(d, "@dir"))


def digest(obj):
    """SHA-256 of tests/test_config.py's canonical form."""
    return hashlib.sha256(json.dumps(obj, sort_keys=True, indent=1).encode()).hexdigest()


def main():
    assert len(sys.argv) == 2 and os.path.isdir(sys.argv[1]), __doc__
    assert rr.lib() is not None, "build oracle/_ref first (make -C oracle)"
    out = {"argv": ARGV, "templates": []}
    with tempfile.TemporaryDirectory() as d:
        for k, (script, target, text) in enumerate(script_templates(sys.argv[1])):
            path = os.path.join(d, "t%d.cfg" % k)
            with open(path, "w", newline="") as f:
                f.write(text)
            argv = [path if a == "@path" else a for a in ARGV]
            out["templates"].append({"script": script, "target": target, "text": text,
                                     "reference_sha256": digest(scrub(rr.dump(cfg_path=path), d)),
                                     "reference_argv_sha256": digest(scrub(rr.dump(argv=argv), d))})
    with open(os.path.join(HERE, "script_templates.json"), "w") as f:
        json.dump(out, f, sort_keys=True, indent=1)
    print("wrote script_templates.json: %d templates" % len(out["templates"]))


if __name__ == "__main__":
    main()
