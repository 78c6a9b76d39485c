"""Writes tests/golden/gtm_player.json: what the reference's own player (decoders/htmljs/gtm.player.js over its
lzma.js, driven by oracle/ref_player.js under node) draws for every case of tests/gtm_player_cases.py and for its
two demo clips -- per frame the SHA-256 of the RGBA framebuffer -- with the SHA-256 and length of each file it was
given.  Needs node, the reference tree ($TILER_REFERENCE, default /root/reference) and the built libANN.so (the
cases are written by its LZMA encoder; no GPU).  The files themselves are not kept: the registry rebuilds the cases,
the demo clips stay in the reference tree.  Run from the repo root: python tests/golden/make_gtm_player_golden.py

Asserted while generating: the player logs no error on any case, plays the frame count and size that went in, and
its whole-clip digests of the demo clips are gtm_demo.json's rendered_sha256 (the test player's)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)
import pyoracle  # noqa: E402
import gtm_player_cases as cases  # noqa: E402

DEMO = os.path.join(os.environ.get("TILER_REFERENCE", "/root/reference"), "docs", "demo")


def played(gtm, name):
    r = pyoracle.ref_player(gtm)
    assert r is not None, "node or the reference's decoders/htmljs is missing"
    assert r["errors"] == [], (name, r["errors"])
    assert r["frames"] == len(r["frame_sha256"]) > 0, name
    return r


def main():
    out = {"cases": {}, "demo": {}}
    for name in cases.NAMES:
        c = cases.case(name)
        r = played(c["data"], name)
        assert (r["width"], r["height"]) == (c["W"], c["H"]), name
        if c["inputs"] is not None:
            assert r["frames"] == c["inputs"]["F"], name
        out["cases"][name] = {"file_sha256": cases.file_sha256(c["data"]), "file_bytes": len(c["data"]),
                              "width": r["width"], "height": r["height"], "frames": r["frames"],
                              "frame_sha256": r["frame_sha256"], "errors": r["errors"]}
    with open(os.path.join(HERE, "gtm_demo.json")) as f:
        demo = json.load(f)
    for name in cases.DEMO_CLIPS:
        r = played(os.path.join(DEMO, name), name)
        assert r["clip_sha256"] == demo[name]["rendered_sha256"], name
        assert (r["frames"], r["width"], r["height"]) == (demo[name]["frames"], demo[name]["width"],
                                                          demo[name]["height"]), name
        out["demo"][name] = {"file_sha256": demo[name]["file_sha256"], "file_bytes": demo[name]["file_bytes"],
                             "width": r["width"], "height": r["height"], "frames": r["frames"],
                             "clip_sha256": r["clip_sha256"], "frame_sha256": r["frame_sha256"],
                             "errors": r["errors"]}
    with open(cases.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for kind in ("cases", "demo"):
        for name, v in out[kind].items():
            print(f"{kind[:4]} {name}: {v['file_bytes']} bytes, {v['width']} x {v['height']}, {v['frames']} frames")


if __name__ == "__main__":
    main()
