"""What a VOC evaluation pass costs (pascal/pascal_eval_darknet.py, csrc/detect.hip) against the per-image way of doing
the same images, on a devkit made by replicating the two fixture images of tests/golden (make_devkit below):

  device    pascal_eval_darknet.evaluate: per batch eval_batch -> forward_u8 -> y2_detect_grid_batch ->
            y2_voc_match_batch, one device-to-host copy, map_from_flags on the host
  per-image the same batches and forward passes, then per image net_utils.decode_yolo_detection (two device-to-host
            copies and a Python loop over S * S * B rows) + voc_eval.detections_from_decode, and voc_eval.voc_map over
            the whole list at the end, at the same confidence threshold (no NMS exists on that path: it scores more rows)
  forward   eval_batch -> forward_u8 alone over the same batches

Wall clock around each pass with a synchronisation before and after; one untimed pass of each first, then the median of
--reps passes.  The network holds its initial values (a plumbing run): the confidences are whatever the initial values
give, so the threshold mainly sets how many rows the post-processing sees, which is what is being timed.  The head runs
on batch statistics (--head-batch-stats): on the moving statistics the initial values grow the activations beyond every
box limit and no path would have a row to score.

    python scripts/bench_device_voc_eval.py --out profiles/device_voc_eval.txt
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECOND_XML = """<annotation><size><width>352</width><height>240</height><depth>3</depth></size>
<object><name>car</name><difficult>0</difficult><bndbox><xmin>1</xmin><ymin>1</ymin><xmax>352</xmax><ymax>240</ymax></bndbox></object>
<object><name>cat</name><difficult>0</difficult><bndbox><xmin>30</xmin><ymin>40</ymin><xmax>120</xmax><ymax>200</ymax></bndbox></object>
<object><name>bird</name><difficult>1</difficult><bndbox><xmin>35</xmin><ymin>45</ymin><xmax>118</xmax><ymax>190</ymax></bndbox></object>
</annotation>
"""


def make_devkit(root, images, image_set="test"):
    """`images` entries alternating between testImg2 (353 x 500, its golden annotation) and testImg1 (352 x 240, three
    hand-made objects, one of them difficult)"""
    golden = os.path.join(ROOT, "tests", "golden")
    voc = os.path.join(root, "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(voc, d), exist_ok=True)
    names = []
    for k in range(images):
        name = "%06d" % (k + 1)
        if k % 2 == 0:
            shutil.copy(os.path.join(golden, "testImg2.jpg"), os.path.join(voc, "JPEGImages", name + ".jpg"))
            shutil.copy(os.path.join(golden, "testImg2Anno.xml"), os.path.join(voc, "Annotations", name + ".xml"))
        else:
            shutil.copy(os.path.join(golden, "testImg1.jpg"), os.path.join(voc, "JPEGImages", name + ".jpg"))
            with open(os.path.join(voc, "Annotations", name + ".xml"), "w") as f:
                f.write(SECOND_XML)
        names.append(name)
    with open(os.path.join(voc, "ImageSets", "Main", image_set + ".txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return root


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--thresh", type=float, default=0.005)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import config as cfg
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.pascal import pascal_eval_darknet as P
    from tensorflow_yolo2_amd.utils import voc_eval
    from tensorflow_yolo2_amd.yolo2_nets import darknet, net_utils
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        fn()                                                   # warm-up: kernel loads, filter packs, allocator
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times), out

    with tempfile.TemporaryDirectory() as tmp:
        kit = make_devkit(os.path.join(tmp, "VOCdevkit"), args.images)
        imdb = DeviceVOC("test", batch_size=args.batch, devkit_path=kit, flipped=False)
        n, size, S, B = args.batch, args.size, args.size // 32, cfg.B
        darknet.set_default_dtype(args.dtype)
        x = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        grid = darknet.darknet19_detection(darknet.darknet19_core(x, is_training=False), 5 * B + 20, is_training=True)
        network = grid.reshape([-1, S, S, 5 * B + 20]).build(training=False)
        entries = len(imdb.entries)
        batches = (entries + n - 1) // n

        def forward_only():
            for k in range(batches):
                images, _ = imdb.eval_batch(size, k * n)
                P.grid_net_forward(network, images, True)

        def device():
            return P.evaluate(network, imdb, size, args.thresh, 0.45, 100, True, head_batch_stats=True)

        def per_image():
            dets, gts = [], []
            for k in range(batches):
                images, valid = imdb.eval_batch(size, k * n)
                out = P.grid_net_forward(network, images, True)
                for j in range(valid):
                    e = imdb.entries[k * n + j]
                    rows = net_utils.decode_yolo_detection(out[j], e['shape'][1], e['shape'][0], 20, S, B, args.thresh)
                    dets += voc_eval.detections_from_decode(k * n + j, rows)
            for i, e in enumerate(imdb.entries):
                gts += [(i, o[4], o[0] - 1, o[1] - 1, o[2] - 1, o[3] - 1, d) for o, d in zip(e['objs'], e['difficult'])]
            return voc_eval.voc_map(dets, gts, use_07_metric=True), len(dets)

        say("VOC evaluation pass: %d images (tests/golden replicated), batch %d, %d x %d, %s, confidence > %g, initial "
            "values; wall clock, median of %d passes after one untimed pass" % (entries, n, size, size, args.dtype,
                                                                                 args.thresh, args.reps))
        t_fwd, _ = timed(forward_only)
        t_dev, r = timed(device)
        t_img, ((m_img, _aps), rows_img) = timed(per_image)
        say("pass                                   seconds   ms/image   detections scored")
        say("forward only (resize + network)        %7.3f   %8.3f" % (t_fwd, 1e3 * t_fwd / entries))
        say("device (detect + NMS + match kernels)  %7.3f   %8.3f   %d (after NMS, <= 100 per image)"
            % (t_dev, 1e3 * t_dev / entries, len(r["rows"]["flag"])))
        say("per image (decode round trips, voc_map) %6.3f   %8.3f   %d (no NMS on that path)"
            % (t_img, 1e3 * t_img / entries, rows_img))
        say("post-processing = pass - forward:  device %.3f s (%.2f x the forward pass), per image %.3f s (%.2f x)"
            % (t_dev - t_fwd, (t_dev - t_fwd) / t_fwd, t_img - t_fwd, (t_img - t_fwd) / t_fwd))
        say("mAP (initial values, meaningless as a score): device %.4f, per image %.4f" % (r["mAP"], m_img))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
