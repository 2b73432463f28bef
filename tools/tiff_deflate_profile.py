"""profiles/tiff_deflate_stage.json: the inflation of a TIFF's Deflate chunks on the device (OCR_DEVICE_TIFF=3) against zlib on
the host, measured with decode_tool --time on one GPU.

    python tools/tiff_deflate_profile.py <out.json>

Inputs, generated here: the 960 x 960 RGB text page of tools/tiff_lzw_profile.py, zlib level 6 with predictor 2, at 16 rows a
strip and as one strip.  Each as one image and as a batch of 64, three runs, medians beside them, next to the host's zlib
figure on one thread and that figure divided by 16."""
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tiff_writer as tw  # noqa: E402
from tiff_lzw_profile import TOOL, text_page, time_file  # noqa: E402


def main():
    out = sys.argv[1]
    rs = np.random.RandomState(960)
    d = tempfile.mkdtemp(prefix="tiffdeflate")
    page = text_page(rs)
    runs, medians = [], []
    keys = ("upload_ms", "pixel_stage_ms", "coded_upload_ms", "inflate_stage_ms", "coded_pixel_stage_ms", "host_inflate_ms_per_image")
    for rps in (16, None):
        path = os.path.join(d, "text_%s.tif" % (rps or "one"))
        open(path, "wb").write(tw.write_tiff(page, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=rps))
        for batch in (1, 64):
            three = [dict(time_file(TOOL, path, batch), image="text", rows_per_strip=rps or 960, file_bytes=os.path.getsize(path)) for _ in range(3)]
            runs += three
            m = {k: statistics.median(r[k] for r in three) for k in keys}
            m.update(image="text", rows_per_strip=rps or 960, batch=batch, chunks=three[0]["chunks"], coded_bytes=three[0]["coded_bytes"], expanded_bytes=three[0]["bytes_in"] // batch)
            # per batch: what the =3 route pays (upload of the coded bytes, the inflate launch with its read-back) against what the
            # =1 route pays for the same chunks (zlib on the host, and the larger upload)
            m["route3_upload_inflate_ms"] = m["coded_upload_ms"] + m["inflate_stage_ms"]
            m["host_zlib_one_thread_ms"] = m["host_inflate_ms_per_image"] * batch
            m["host_zlib_one_thread_over_16_ms"] = m["host_zlib_one_thread_ms"] / 16
            m["route1_inflate_upload_ms"] = m["host_zlib_one_thread_ms"] + m["upload_ms"]
            m["route1_on_16_host_threads_ms"] = m["host_inflate_ms_per_image"] * batch / min(16, batch) + m["upload_ms"]
            medians.append(m)
            print(json.dumps(m), flush=True)
    json.dump({"what": __doc__, "medians": medians, "runs": runs}, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
