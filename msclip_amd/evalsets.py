"""Readers of the zero-shot evaluation sets that are not ImageFolder trees (reference lib/evaluation/dataset.py:11-116, selected by
DATASET.DATASET in tools/zero_shot.py:208-213).  Each returns the list of (image path, label) that zeroshot.evaluate takes as
`items`: the label is a multi-hot list for VOC2007 (TEST.METRIC 11point_mAP) and 0 / 1 for Hateful Memes (roc_auc).  Reading the
images is zeroshot.ImagePipeline's business.
"""
import json
import os

VOC_SUFFIX = {"train": ("train", "VOCdevkit", "VOC2007"), "val": ("train", "VOCdevkit", "VOC2007"),
              "test": ("test", "VOCdevkit 2", "VOC2007")}                  # dataset.py:22-29 (the test archive unpacks beside the other)
HATEFUL_FILE = {"train": "train.jsonl", "val": "dev_seen.jsonl"}           # dataset.py:105-110


def voc2007_categories(root, image_set):
    """The sorted category names of ImageSets/Main/<category>_<image_set>.txt under the set's VOC2007 directory (for the released
    archives: the twenty names of dataset.py:50-52, in that order)."""
    if image_set not in VOC_SUFFIX:
        raise ValueError("Incorrect image set!")
    main = os.path.join(root, *VOC_SUFFIX[image_set], "ImageSets", "Main")
    return sorted(f.split("_")[0] for f in os.listdir(main) if f.endswith("_" + image_set + ".txt"))


def voc2007_items(root, image_set="test"):
    """[(path of JPEGImages/<id>.jpg, multi-hot list over voc2007_categories)], sorted by image id.  A line of a category file is
    "<id> <flag>" with the flag in columns 7-8: 1 marks a positive, 0 (difficult) and -1 are negatives, as is an image that a
    category's file does not list (dataset.py:56-69)."""
    cats = voc2007_categories(root, image_set)
    base = os.path.join(root, *VOC_SUFFIX[image_set])
    labels = {}
    for ci, cat in enumerate(cats):
        with open(os.path.join(base, "ImageSets", "Main", f"{cat}_{image_set}.txt")) as f:
            for line in f:
                if not line.strip():
                    continue
                row = labels.setdefault(line[:6], [0] * len(cats))
                flag = line[7:9]
                if not flag or int(flag) == 1:                             # (dataset.py:64-68: no flag field counts as a positive)
                    row[ci] = 1
    return [(os.path.join(base, "JPEGImages", idx + ".jpg"), labels[idx]) for idx in sorted(labels)]


def hatefulmemes_items(root, image_set="val"):
    """[(path of the record's "img", its "label")] of dev_seen.jsonl (val) or train.jsonl (train), in file order."""
    if image_set not in HATEFUL_FILE:
        raise ValueError(f"Incorrect image_set value: {image_set}!")
    items = []
    with open(os.path.join(root, HATEFUL_FILE[image_set])) as f:
        for line in f:
            if line.strip():
                rec = json.loads(line)
                items.append((os.path.join(root, rec["img"]), int(rec["label"])))
    return items
