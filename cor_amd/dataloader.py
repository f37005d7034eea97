"""Validation data path of the reference on the HIP pre-processing kernels.

Mirrors utils/dataloader.py:244-413 (class VaildingDataset, get_vaild_loader): same CSV schema
(Id, Query_img, Query_mask, Support_img, Support_mask, Text, Compose, Dataset, Target, query_cat; rows with Compose != 0 are
dropped), same directory layout (<dataset_path>/<Dataset>/image/<file>, .../mask/<Target>/<Query_mask>, .../mask/sup/
<Support_mask>), same batch dict keys. MI355X-first split of the work: DataLoader workers only DECODE files (PIL, host);
`Resize -> ToTensor -> Normalize` runs on the GPU in the collate step of the main process (cor_amd/preprocess.py: Pillow's
antialiased bilinear resize bit-exactly, csrc/preproc.hip), so a batch arrives on the device already at model size.
The SigLIP tokenizer is resolved by name through open_clip in the reference (an HF-hub download): here `text_tokenizer` is a
callable str -> LongTensor[64] (cor_amd.tokenizer.siglip_tokenizer builds one from a local sentencepiece model file)."""
from __future__ import annotations

import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import preprocess as P

CSV_COLUMNS = ["Id", "Query_img", "Query_mask", "Support_img", "Support_mask", "Text", "Compose", "Dataset", "Target", "query_cat"]


def read_pairs_csv(csv_path):
    """ref: utils/dataloader.py:258-261 - pandas frame of the pairs with Compose == 0."""
    import pandas as pd
    df = pd.read_csv(csv_path)
    missing = [c for c in CSV_COLUMNS if c not in df.columns]
    if missing:
        raise ValueError(f"{csv_path}: missing CSV columns {missing}")
    return df[df["Compose"] == 0].reset_index(drop=True)


class VaildingDataset(Dataset):
    """ref: utils/dataloader.py:244-369. __getitem__ returns DECODED uint8 arrays (no resize: that happens on the GPU in
    `collate_on_device`) plus the reference's metadata fields."""

    def __init__(self, csv_path, dataset_path, support_img_size=384, text_tokenizer=None):
        self.dataset_csv = read_pairs_csv(csv_path)
        self.dataset_path = dataset_path
        self.query_img_size = 1024                     # "use sam pretrain can't change" (dataloader.py:262)
        self.support_img_size = support_img_size
        self.support_mask_size = support_img_size
        if text_tokenizer is None or isinstance(text_tokenizer, str):
            raise ValueError("text_tokenizer must be a callable str -> LongTensor[ctx] (the reference resolves a hub tokenizer by "
                             "name, which needs network access); see cor_amd.tokenizer")
        self.siglip_text_tokenizer = text_tokenizer
        self.dataset_size = len(self.dataset_csv)

    @staticmethod
    def rgb_loader(path):
        from PIL import Image
        with open(path, "rb") as f:
            return np.asarray(Image.open(f).convert("RGB"))

    @staticmethod
    def binary_loader(path):
        from PIL import Image
        with open(path, "rb") as f:
            return np.asarray(Image.open(f).convert("L"))

    def __len__(self):
        return self.dataset_size

    def __getitem__(self, idx):
        row = self.dataset_csv.iloc[idx]
        ds, tgt = row["Dataset"], row["Target"]
        root = os.path.join(self.dataset_path, ds)
        text_string = row["Text"]
        tokens = torch.as_tensor(self.siglip_text_tokenizer(text_string)).reshape(-1).to(torch.int64)
        return {
            "pair_id": row["Id"],
            "query_img_u8": self.rgb_loader(os.path.join(root, "image", row["Query_img"])),
            "query_mask_u8": self.binary_loader(os.path.join(root, "mask", str(tgt), row["Query_mask"])),
            "support_img_u8": self.rgb_loader(os.path.join(root, "image", row["Support_img"])),
            "support_mask_u8": self.binary_loader(os.path.join(root, "mask", "sup", row["Support_mask"])),
            "text": tokens, "text_string": text_string, "compose": int(row["Compose"]), "dataset": ds, "target": tgt,
            "query_cat": row["query_cat"], "query_img_name": row["Query_img"], "query_mask_name": row["Query_mask"],
            "support_img_name": row["Support_img"], "support_mask_name": row["Support_mask"],
        }


class collate_on_device:
    """Stacks a list of samples into the reference's batch dict; the four image fields are resized / normalised on `device`
    (utils/dataloader.py:266-293: Resize -> ToTensor -> Normalize for images, Resize -> ToTensor for masks)."""

    def __init__(self, device, support_img_size=384, query_img_size=1024):
        self.device = torch.device(device)
        self.q_img, self.q_mask = P.ImageTransform(query_img_size), P.MaskTransform(query_img_size)
        self.s_img, self.s_mask = P.ImageTransform(support_img_size), P.MaskTransform(support_img_size)

    def __call__(self, samples):
        dev = self.device
        up = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)               # noqa: E731 (PIL hands out read-only arrays)
        out = {
            "query_img": torch.stack([self.q_img(up(s["query_img_u8"])) for s in samples]),
            "query_mask": torch.stack([self.q_mask(up(s["query_mask_u8"])) for s in samples]),
            "support_img": torch.stack([self.s_img(up(s["support_img_u8"])) for s in samples]),
            "support_mask": torch.stack([self.s_mask(up(s["support_mask_u8"])) for s in samples]),
            "text": torch.stack([s["text"] for s in samples]).to(dev),
        }
        for k in ("pair_id", "text_string", "compose", "dataset", "target", "query_cat", "query_img_name", "query_mask_name",
                  "support_img_name", "support_mask_name"):
            out[k] = [s[k] for s in samples]
        return out


def get_vaild_loader(csv_path, dataset_path, support_img_size=384, text_tokenizer=None, batch_size=8, shuffle=False, num_workers=12,
                     pin_memory=True, prefetch_factor=4, worker_init_fn=None, device="cuda"):
    """ref: utils/dataloader.py:372-413 (same arguments; `device` is where the collate step runs the resize kernels).
    pin_memory is accepted for signature compatibility: the collate step already produces device tensors."""
    dataset = VaildingDataset(csv_path, dataset_path, support_img_size=support_img_size, text_tokenizer=text_tokenizer)
    kw = dict(dataset=dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, worker_init_fn=worker_init_fn,
              collate_fn=_HostCollate())
    if num_workers > 0:
        kw["prefetch_factor"] = prefetch_factor
    return _DeviceLoader(DataLoader(**kw), collate_on_device(device, support_img_size, dataset.query_img_size))


class _HostCollate:
    """Workers hand over the decoded samples as a plain list (variable image sizes cannot be stacked on the host)."""

    def __call__(self, samples):
        return samples


class _DeviceLoader:
    """Iterates the host DataLoader and runs the device collate in the consuming (main) process."""

    def __init__(self, loader, collate):
        self.loader, self.collate, self.dataset = loader, collate, loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for samples in self.loader:
            yield self.collate(samples)


def gallery_labels(csv_path, column="Target"):
    """One int32 label per gallery row, for the rows gallery_batches yields and in its order (read_pairs_csv): ids of the names in
    `column` by first appearance. Returns (labels int32[n], names) with names[label] the column value. column="Target" (the object
    class) or "Dataset" restrict a filtered search with mode "eq"; column="Query_img" gives image ids, to exclude a query's own image
    with mode "ne"."""
    import pandas as pd
    df = read_pairs_csv(csv_path)
    if column not in df.columns:
        raise ValueError(f"gallery_labels: no column {column!r} in {csv_path}")
    codes, names = pd.factorize(df[column], sort=False)
    return torch.from_numpy(np.asarray(codes, dtype=np.int32)), list(names)


def gallery_batches(csv_path, dataset_path, batch_size=8, device="cuda", num_workers=0):
    """Offline gallery builder input: yields {"query_img", "query_mask"} device batches for
    cor_amd.retrieval.build_gallery from the same CSV schema (one gallery row per CSV pair: query image + query mask)."""
    class _G(Dataset):
        def __init__(self):
            self.df = read_pairs_csv(csv_path)

        def __len__(self):
            return len(self.df)

        def __getitem__(self, i):
            row = self.df.iloc[i]
            root = os.path.join(dataset_path, row["Dataset"])
            return {"q": VaildingDataset.rgb_loader(os.path.join(root, "image", row["Query_img"])),
                    "m": VaildingDataset.binary_loader(os.path.join(root, "mask", str(row["Target"]), row["Query_mask"]))}

    dev = torch.device(device)
    q_img, q_mask = P.ImageTransform(1024), P.MaskTransform(1024)
    up = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)                   # noqa: E731
    for samples in DataLoader(_G(), batch_size=batch_size, shuffle=False, num_workers=num_workers, collate_fn=_HostCollate()):
        yield {"query_img": torch.stack([q_img(up(s["q"])) for s in samples]),
               "query_mask": torch.stack([q_mask(up(s["m"])) for s in samples])}


def gallery_groups(csv_path):
    """One int32 group id per gallery row (the rows of read_pairs_csv, in its order, as gallery_labels): ids of the source IMAGE, i.e. of
    the pair (Dataset, Query_img), by first appearance - two datasets that both hold a `0001.jpg` get two ids. Returns
    (groups int32[n], keys) with keys[id] = (Dataset, Query_img). The ids GalleryShard(groups=...), save_gallery(groups=...) and
    search(distinct=True) consume."""
    df = read_pairs_csv(csv_path)
    ids, keys, out = {}, [], np.empty(len(df), dtype=np.int32)
    for i, key in enumerate(zip(df["Dataset"].tolist(), df["Query_img"].tolist())):
        if key not in ids:
            ids[key] = len(keys)
            keys.append(key)
        out[i] = ids[key]
    return torch.from_numpy(out), keys


def plan_region_batches(groups, images_per_batch, max_regions=None):
    """Batches for the multi-region gallery builder, from one group (image) id per CSV row: a list of batches, each a list of
    (image_id, [row indices]). Images come in order of first appearance and an image's rows in CSV order, wherever they stand in the
    CSV; a batch holds at most `images_per_batch` images and, when `max_regions` is given, at most that many rows. Only an image with
    more than `max_regions` rows of its own is split, over consecutive batches (it is then encoded once per piece); any other image
    that does not fit the room left opens the next batch. Every row appears exactly once."""
    images_per_batch = int(images_per_batch)
    if images_per_batch < 1 or (max_regions is not None and int(max_regions) < 1):
        raise ValueError("plan_region_batches: images_per_batch and max_regions must be >= 1")
    by_image = {}
    for i, g in enumerate(torch.as_tensor(groups).reshape(-1).tolist()):
        by_image.setdefault(int(g), []).append(i)
    pieces = []
    for g, rows in by_image.items():                            # dicts keep insertion order: first appearance
        step = len(rows) if max_regions is None else int(max_regions)
        pieces += [(g, rows[j:j + step]) for j in range(0, len(rows), step)]
    batches, cur, n = [], [], 0
    for g, rows in pieces:
        if cur and (len(cur) == images_per_batch or (max_regions is not None and n + len(rows) > int(max_regions))):
            batches.append(cur)
            cur, n = [], 0
        cur.append((g, rows))
        n += len(rows)
    if cur:
        batches.append(cur)
    return batches


class _RegionBatches(Dataset):
    """Item i: the decoded files of batch i of a plan_region_batches plan (every image of the batch once, every mask once)."""

    def __init__(self, df, dataset_path, plan):
        self.df, self.dataset_path, self.plan = df, dataset_path, plan

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        out = []
        for g, rows in self.plan[i]:
            first = self.df.iloc[rows[0]]
            root = os.path.join(self.dataset_path, first["Dataset"])
            masks = []
            for r in rows:
                row = self.df.iloc[r]
                masks.append(VaildingDataset.binary_loader(os.path.join(root, "mask", str(row["Target"]), row["Query_mask"])))
            out.append({"id": g, "rows": rows, "q": VaildingDataset.rgb_loader(os.path.join(root, "image", first["Query_img"])), "m": masks})
        return out


def _identity(x):
    return x


def gallery_region_batches(csv_path, dataset_path, batch_size=8, device="cuda", num_workers=0, max_regions=None, grid=64):
    """Input of cor_amd.retrieval.build_gallery_regions from the CSV schema of gallery_batches: every distinct image (Dataset, Query_img)
    is decoded and resized ONCE, each of its masks once; yields {"query_img" f32[B,3,1024,1024], "region_masks" f32[R,1,grid,grid],
    "region_offsets" int32[B+1], "image_ids" (gallery_groups' ids), "row_index" (the CSV row of each region)} with B <= batch_size images
    (and R <= max_regions regions when given: plan_region_batches). With row_index the builder returns its rows in CSV order, the
    layout of build_gallery(model, gallery_batches(...)) and of gallery_labels / gallery_groups. Every mask is reduced to the encoder's
    token grid (`grid` = image size / patch size = 64 for SAM; ops.bilinear, per plane what the batched call gives) as soon as it is
    resized, so device memory for masks does not grow with 1024^2 x regions."""
    from . import ops
    df = read_pairs_csv(csv_path)
    groups, _ = gallery_groups(csv_path)
    plan = plan_region_batches(groups, batch_size, max_regions)
    dev = torch.device(device)
    q_img, q_mask = P.ImageTransform(1024), P.MaskTransform(1024)
    up = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)                   # noqa: E731
    for items in DataLoader(_RegionBatches(df, dataset_path, plan), batch_size=None, shuffle=False, num_workers=num_workers, collate_fn=_identity):
        imgs, planes, offsets, ids, index = [], [], [0], [], []
        for it in items:
            imgs.append(q_img(up(it["q"])))
            for m in it["m"]:
                planes.append(ops.bilinear(q_mask(up(m)).reshape(1, 1, 1024, 1024).contiguous(), grid, grid)[0])
            offsets.append(offsets[-1] + len(it["m"]))
            ids.append(it["id"])
            index += list(it["rows"])
        yield {"query_img": torch.stack(imgs), "region_masks": torch.stack(planes),
               "region_offsets": torch.tensor(offsets, dtype=torch.int32), "image_ids": torch.tensor(ids, dtype=torch.int32),
               "row_index": torch.tensor(index, dtype=torch.int64)}
