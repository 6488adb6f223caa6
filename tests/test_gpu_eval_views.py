"""Classifier validation from the device pool on the GPU: DeviceCls.eval_views bit for bit against the host reference
eval_views.view_images, and the test / predict / train scripts' new flags.  The views are compared by equality; with one
view the scores are ordered on the logits, so the scripts' ranks are recounted exactly in numpy."""
import numpy as np
import pytest

from test_cls_augment_host import write_list

pytestmark = pytest.mark.gpu

LIST_SHAPES = [(40, 52), (64, 48), (33, 33), (90, 70), (37, 53), (50, 120), (64, 64)]


def _write(tmp_path):
    items, imgs = write_list(tmp_path, LIST_SHAPES)
    lst = tmp_path / "val.txt"
    lst.write_text("".join("%s %d\n" % it for it in items))
    return items, imgs, str(lst)


def test_eval_views_equal_the_host_views_slot_by_slot(tmp_path):
    import torch
    from tensorflow_yolo2_amd.img_dataset import eval_views as EV
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    items, imgs, _ = _write(tmp_path)
    dev = DeviceCls(items, 3)
    before = [dev.eval_batch(64, start)[0].clone() for start in (0, 3, 6)]
    for size in (32, 64):
        for views in ("stretch", "centre", "ten"):
            V = EV.VIEWS[views]
            for start in (0, 3, 6):
                images, valid = dev.eval_views(size, start, views)
                torch.cuda.synchronize()
                assert images.dtype == torch.uint8 and tuple(images.shape) == (3 * V, size, size, 3)
                assert valid == min(3, 7 - start)
                got = images.cpu().numpy()
                idx = np.minimum(np.arange(start, start + 3), 6)
                for b, e in enumerate(idx):
                    rows = EV.view_rows([LIST_SHAPES[e]], size, views)[0]
                    want = EV.view_images(imgs[e], rows, size)
                    assert (got[b * V:(b + 1) * V] == want).all(), (size, views, start, b)
                assert dev.labels_of(start).cpu().numpy().tolist() == [items[i][1] for i in idx]
    # other arguments: the margin and the fill reach the rows and the launch
    images, _ = dev.eval_views(32, 3, "ten", margin=0, fill=9)
    rows = EV.view_rows([LIST_SHAPES[3]], 32, "ten", margin=0)[0]
    assert (images.cpu().numpy()[:10] == EV.view_images(imgs[3], rows, 32, fill=9)).all()
    for start, img in zip((0, 3, 6), before):                   # eval_batch returns what it returned before
        assert torch.equal(dev.eval_batch(64, start)[0], img)
    with pytest.raises(ValueError, match="views"):
        dev.eval_views(32, 0, "five")
    with pytest.raises(ValueError, match="multiple of 32"):
        dev.eval_views(48, 0, "centre")
    with pytest.raises(IndexError):
        dev.eval_views(32, 7, "centre")
    from tensorflow_yolo2_amd.img_dataset.augment_cls import ClsAugment
    with pytest.raises(ValueError, match="augment=None"):
        DeviceCls(items, 3, augment=ClsAugment()).eval_views(32, 0, "centre")


def test_test_script_centre_view_counts_what_numpy_counts(tmp_path, capsys):
    """seven images at batch 3: the remainder path.  One view: the order is the logits', so the recount is exact"""
    import torch
    from tensorflow_yolo2_amd.imagenet import imagenet_test_darknet
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    items, _, lst = _write(tmp_path)
    r = imagenet_test_darknet.main(["--image-list", lst, "--device-data", "--batch", "3", "--views", "centre",
                                    "--topk", "5", "--dtype", "f32"])
    out = capsys.readouterr().out
    assert r["images"] == 7 and r["ranks"].dtype == np.int32 and r["ranks"].shape == (7,)
    assert out.count("batch ") >= 3 and "top-5" in out
    net, dev = r["network"], DeviceCls(items, 3)
    ranks = []
    for start in (0, 3, 6):
        images, valid = dev.eval_views(224, start, "centre")
        logits = net.forward(images, False, False).cpu().numpy().astype(np.float64)
        labels = dev.labels_of(start).cpu().numpy()
        for b in range(valid):
            order = np.argsort(-logits[b], kind="stable")
            ranks.append(order.tolist().index(labels[b]))
    assert r["ranks"].tolist() == ranks
    assert r["top1"] == sum(x == 0 for x in ranks) / 7.0 and r["topk"] == sum(x < 5 for x in ranks) / 7.0
    assert r["accuracy"] == r["top1"]
    with pytest.raises(SystemExit):
        imagenet_test_darknet.main(["--image-list", lst, "--views", "centre"])      # needs --device-data
    with pytest.raises(SystemExit):
        imagenet_test_darknet.main(["--image-list", lst, "--topk", "5"])


def test_test_script_ten_views(tmp_path):
    from tensorflow_yolo2_amd.imagenet import imagenet_test_darknet
    _, _, lst = _write(tmp_path)
    r = imagenet_test_darknet.main(["--image-list", lst, "--device-data", "--batch", "2", "--views", "ten",
                                    "--dtype", "f32"])
    assert r["network"].batch == 20 and r["images"] == 7
    assert r["topk"] >= r["top1"] and len(r["ranks"]) == 7
    assert ((r["ranks"] >= 0) & (r["ranks"] <= 1000)).all()


def test_predict_script_centre_view(tmp_path):
    from tensorflow_yolo2_amd.imagenet import imagenet_predict_darknet
    from tensorflow_yolo2_amd.utils.score_views import score_views_ref
    items, _, _ = _write(tmp_path)
    r = imagenet_predict_darknet.main([items[5][0], "--views", "centre", "--dtype", "f32"])
    logits = r["logits"].cpu().numpy()
    assert logits.shape == (1, 1000)
    idx, val, _, _, _ = score_views_ref(logits, views=1, k=5)
    assert r["predictions"] == idx[0].tolist()
    dmax = float(logits.max()) - float(logits.min())            # the bound of test_gpu_score_views.py for this case
    np.testing.assert_allclose(r["values"], val[0], rtol=(2 * dmax + 1000 + 1 + 8) * 2.0 ** -24, atol=0)
    with pytest.raises(SystemExit):
        imagenet_predict_darknet.main([items[5][0], "--views", "centre", "--raw-pixels"])


def _same_loss(la, lb, n):
    """the loss scalar of y2_softmax_cross_entropy is an atomic float32 sum of n row terms (test_gpu_device_cls.py says
    why two equal steps may differ): (n - 1) ulp between two orders"""
    assert np.isfinite(la) and np.isfinite(lb)
    assert abs(np.float32(la) - np.float32(lb)) <= (n - 1) * np.spacing(np.float32(max(la, lb))), (la, lb)


def test_train_script_without_val_views_validates_as_before(tmp_path, monkeypatch, capsys):
    """--val-views absent: the validation batch is eval_batch's stretch through the trainer's own network and the
    existing loss / accuracy kernels -- no view batch, no scoring launch; given, the views are scored"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.imagenet import imagenet_train_darknet
    from tensorflow_yolo2_amd.img_dataset import device_cls
    _, _, lst = _write(tmp_path)
    calls = {"eval_views": 0, "eval_batch": 0, "score_views": 0}

    def counted(owner, name):
        real = getattr(owner, name)

        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, f)
    counted(device_cls.DeviceCls, "eval_views")
    counted(device_cls.DeviceCls, "eval_batch")
    counted(E, "score_views")
    argv = ["--image-list", lst, "--val-list", lst, "--device-data", "--iters", "25", "--batch", "4", "--size", "64",
            "--dtype", "f32"]
    r1 = imagenet_train_darknet.main(argv)
    out1 = capsys.readouterr().out
    assert calls == {"eval_views": 0, "eval_batch": 1, "score_views": 0} and out1.count("###validation loss") == 1
    r2 = imagenet_train_darknet.main(argv + ["--val-views", "stretch"])
    out2 = capsys.readouterr().out
    assert calls == {"eval_views": 0, "eval_batch": 2, "score_views": 0}
    assert torch.equal(r1["trainer"].net.params.view(torch.int32), r2["trainer"].net.params.view(torch.int32))
    for (l1, a1), (l2, a2) in zip(r1["log"], r2["log"]):
        assert a1 == a2
        _same_loss(l1, l2, 4)
    v1, v2 = ([l for l in o.splitlines() if l.startswith("###validation")][0].split(", take")[0] for o in (out1, out2))
    assert v1.split("acc:")[1] == v2.split("acc:")[1]
    r3 = imagenet_train_darknet.main(argv + ["--val-views", "ten"])
    out3 = capsys.readouterr().out
    assert calls == {"eval_views": 1, "eval_batch": 2, "score_views": 1} and out3.count("###validation loss") == 1
    assert torch.equal(r1["trainer"].net.params.view(torch.int32), r3["trainer"].net.params.view(torch.int32))
    with pytest.raises(SystemExit):
        imagenet_train_darknet.main(["--iters", "1", "--val-views", "centre"])
