"""profiles/tiff_lzw_stage.json: the TIFF chunk expansion on the device (OCR_DEVICE_TIFF=2) against the host's, measured with
decode_tool --time on one GPU.

    python tools/tiff_lzw_profile.py <out.json> [--parent <decode_tool of the parent commit>]

Inputs, generated here: a 960 x 960 RGB text page (black strokes on white: long LZW strings) and a photographic image (smooth
fields with noise: short strings), LZW with predictor 2, at 16 rows a strip and as one strip.  Each as one image and as a batch of
64, three runs, medians beside them.  --parent: the =1 route's pixel stage of this build against the parent commit's, six
alternating runs each."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_writer as tw  # noqa: E402

TOOL = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host", "decode_tool")


def text_page(rs, n=960):
    page = np.full((n, n, 3), 255, np.int64)
    for y in range(40, n - 40, 28):      # lines of words of strokes
        x = 40
        while x < n - 60:
            for _ in range(rs.randint(2, 9)):
                w, h = rs.randint(2, 5), rs.randint(8, 18)
                page[y + 18 - h:y + 18, x:x + w] = 0
                if rs.randint(2):
                    page[y + 18 - h:y + 18 - h + 2, x:x + 7] = 0
                x += rs.randint(7, 11)
            x += 12
    return page


def photo(rs, n=960):
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    chans = [128 + 90 * np.sin(x / (40 + 17 * c) + c) * np.cos(y / (55 - 9 * c)) + rs.normal(0, 6, (n, n)) for c in range(3)]
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.int64)


def time_file(tool, path, batch, iters=10):
    r = subprocess.run([tool, "--time", str(iters), path] + ([str(batch)] if batch > 1 else []), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    out = sys.argv[1]
    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    rs = np.random.RandomState(960)
    d = tempfile.mkdtemp(prefix="tifflzw")
    inputs = []
    for name, img in (("text", text_page(rs)), ("photo", photo(rs))):
        for rps in (16, None):
            path = os.path.join(d, "%s_%s.tif" % (name, rps or "one"))
            open(path, "wb").write(tw.write_tiff(img, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=rps))
            inputs.append((name, rps or 960, path))
    runs, medians = [], []
    keys = ("upload_ms", "pixel_stage_ms", "coded_upload_ms", "expand_stage_ms", "coded_pixel_stage_ms", "host_scan_ms_per_image", "host_expand_ms_per_image")
    for name, rps, path in inputs:
        for batch in (1, 64):
            three = [dict(time_file(TOOL, path, batch), image=name, rows_per_strip=rps, file_bytes=os.path.getsize(path)) for _ in range(3)]
            runs += three
            m = {k: statistics.median(r[k] for r in three) for k in keys}
            m.update(image=name, rows_per_strip=rps, batch=batch, chunks=three[0]["chunks"], coded_bytes=three[0]["coded_bytes"], expanded_bytes=three[0]["bytes_in"] // batch)
            # the rule for the default, per batch: what the =2 route pays (scan, upload, expansion) against what the =1 route pays
            # for the same chunks (tiff::expand - tiff::parse does not scan - and the larger upload), the host on one thread
            m["route2_scan_upload_expand_ms"] = m["host_scan_ms_per_image"] * batch + m["coded_upload_ms"] + m["expand_stage_ms"]
            m["route1_expand_upload_ms"] = m["host_expand_ms_per_image"] * batch + m["upload_ms"]
            m["route1_on_16_host_threads_ms"] = m["host_expand_ms_per_image"] * batch / min(16, batch) + m["upload_ms"]
            m["route2_on_16_host_threads_ms"] = m["host_scan_ms_per_image"] * batch / min(16, batch) + m["coded_upload_ms"] + m["expand_stage_ms"]
            medians.append(m)
            print(json.dumps(m), flush=True)
    ab = None
    if parent:
        path = inputs[0][2]
        mine, theirs = [], []
        for _ in range(6):
            mine.append(time_file(TOOL, path, 64)["pixel_stage_ms"])
            theirs.append(time_file(parent, path, 64)["pixel_stage_ms"])
        ab = {"what": "pixel_stage_ms of the =1 route, 960 x 960 text page at 16 rows a strip, batch 64, alternating runs", "this_build": mine, "parent_commit": theirs,
              "median_this_build": statistics.median(mine), "median_parent_commit": statistics.median(theirs),
              "spread_this_build": max(mine) - min(mine), "spread_parent_commit": max(theirs) - min(theirs)}
        print(json.dumps(ab), flush=True)
    json.dump({"what": __doc__, "medians": medians, "pixel_stage_against_parent": ab, "runs": runs}, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
