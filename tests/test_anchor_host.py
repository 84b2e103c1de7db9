"""The host-only parts of other_utils/anchor_cluster.py: the cfg rewrite, the two label readers (the `.shapes` cache
included) and the refusals that need no device.  No GPU."""
import os

import numpy as np
import pytest

from other_utils import anchor_cluster as A


def test_change_cfg_file_anchors_rewrites_every_anchors_line(tmp_path, monkeypatch):
    cfg = tmp_path / "net.cfg"
    cfg.write_text("[net]\nwidth=512\n\n[yolo]\nmask = 0,1,2\nanchors = 1,2, 3,4, 5,6\nclasses=1\n\n[yolo]\nanchors=9,9\nnum=3")
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return np.array([[10.9, 13.2], [30.0, 61.7], [116.4, 90.99]])
    monkeypatch.setattr(A, "anchor_cluster", fake)
    k = A.change_cfg_file_anchors(str(cfg), n=3, gen=5)
    assert seen == {"n": 3, "gen": 5} and k.shape == (3, 2)
    new = "anchors = 10, 13, 30, 61, 116, 90"
    assert cfg.read_text() == "[net]\nwidth=512\n\n[yolo]\nmask = 0,1,2\n%s\nclasses=1\n\n[yolo]\n%s\nnum=3" % (new, new)


def test_yolo_dataset_labels_and_the_shapes_cache(tmp_path):
    from PIL import Image
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir()
    lab_dir.mkdir()
    sizes = [(64, 48), (32, 40), (20, 10)]
    names = []
    for i, (w, h) in enumerate(sizes):
        Image.new("RGB", (w, h)).save(str(img_dir / ("f%d_visible.jpg" % i)))
        names.append(str(img_dir / ("f%d.jpg" % i)))
    (lab_dir / "f0.txt").write_text("0 0.5 0.5 0.25 0.5\n0 0.2 0.2 0.1 0.125\n")
    (lab_dir / "f1.txt").write_text("0 0.5 0.5 0.5 0.75\n")               # f2 has no label file
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(names))
    d = A.YOLODatasetLabels(train_data_txt=str(lst))
    assert len(d) == 3 and d.img_files[0].endswith("f0_visible.jpg") and d.label_files[0] == str(lab_dir / "f0.txt")
    shapes, wh = d.get_info()
    assert shapes.tolist() == [[64, 48], [32, 40], [20, 10]] and shapes.dtype == np.float64
    assert [b.shape for b in wh] == [(2, 2), (1, 2), (0, 2)] and wh[0].dtype == np.float32
    assert np.array_equal(wh[0], np.array([[0.25, 0.5], [0.1, 0.125]], np.float32))
    cache = tmp_path / "train.shapes"
    assert cache.read_text().split() == ["64", "48", "32", "40", "20", "10"]
    # the cache is what is read the second time: change it and remove the images
    cache.write_text("640 480\n320 400\n200 100\n")
    for n in names:
        os.remove(n.replace(".jpg", "_visible.jpg"))
    assert A.YOLODatasetLabels(train_data_txt=str(lst)).get_info()[0].tolist() == [[640, 480], [320, 400], [200, 100]]
    with pytest.raises(FileNotFoundError):
        A.YOLODatasetLabels(train_data_txt=str(tmp_path / "absent.txt"))


VOC_XML = """<annotation><folder>x</folder><filename>%s.jpg</filename>
<size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"""
VOC_OBJ = "<object><name>person</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"


def test_voc_dataset_labels(tmp_path):
    root = tmp_path / "voc"
    (root / "Annotations").mkdir(parents=True)
    (root / "ImageSets" / "Main").mkdir(parents=True)
    (root / "Annotations" / "a.xml").write_text(VOC_XML % ("a", 100, 50, VOC_OBJ % (10, 5, 60, 30) + VOC_OBJ % (0, 0, 100, 50)))
    (root / "Annotations" / "b.xml").write_text(VOC_XML % ("b", 80, 40, ""))              # no object: left out
    (root / "Annotations" / "c.xml").write_text(VOC_XML % ("c", 200, 100, VOC_OBJ % (20, 10, 40, 60)))
    (root / "ImageSets" / "Main" / "train.txt").write_text("a\nb\n\nc\n")
    d = A.VOCDatasetLabels(str(root), txt_name="train.txt")
    assert len(d) == 3
    im_wh, boxes = d.get_info()
    assert im_wh == [[100, 50], [200, 100]]
    assert boxes == [[[0.5, 0.5], [1.0, 1.0]], [[0.1, 0.5]]]
    with pytest.raises(AssertionError):
        A.VOCDatasetLabels(str(root), txt_name="absent.txt")
    (root / "ImageSets" / "Main" / "bad.txt").write_text("a\nmissing\n")
    with pytest.raises(AssertionError):
        A.VOCDatasetLabels(str(root), txt_name="bad.txt")


def test_refusals_that_need_no_device():
    wh = np.exp(np.random.RandomState(0).randn(20, 2)).astype(np.float32) + 2
    with pytest.raises(NotImplementedError, match="np.median"):
        A.k_means(wh, 3, dist=np.mean)
    with pytest.raises(ValueError):
        A.evolve_anchors(wh, wh[:3], fitness="anchors")
    with pytest.raises(ValueError):
        A.evolve_anchors(wh, wh[:3], window=0)
    with pytest.raises(ValueError):
        A.anchor_cluster(wh=wh, fitness="neither")
    assert A.exif_size(type("I", (), {"size": (3, 4), "_getexif": lambda self: None})()) == (3, 4)
