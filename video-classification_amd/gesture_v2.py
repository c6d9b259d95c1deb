"""The v2 part-box recipe of the reference (new_feature_test.py:470-979) on the engine.

What it is: SlowFast with a 5-channel slow pathway (RGB + DensePose UV) and a 2-channel fast pathway (gray optical flow),
``init_my_slowfast(cfg, (5, 2), (64, 8))``, trained with SGD (momentum 0.9) on clips cropped to the union of chosen
DensePose part boxes over the clip's frames and resized to MODEL.INPUT_SIZE.

What differs from the reference, and why:
  * the dataset (``ChalearnGestureFrames``) samples frames and boxes exactly as ``ChalearnGestureDataset`` but hands over
    the uncropped uint8 frames (T, H, W, 7) = [R, G, B, U, V, F0, F1] and the box; the crop, ``/255`` and the bilinear
    ``Resize`` run on the device in one ``sfk_roi_resize`` launch (``input_pipeline.RoiResize``).  The resize is pinned
    to ``torch.nn.functional.interpolate``, which torchvision's tensor ``Resize`` calls; torchvision itself is unpinned
    (not installed here).  MODEL.RESIZE_ANTIALIAS picks its antialias flag: True is torchvision >= 0.17, False older;
  * ``ModelManager.prepare_data`` still takes the reference loader's float batch {'rgb', 'uv', 'flow', 'label'};
  * the Trainer is ``train.Trainer`` (checkpoints, device-side eval aggregation, one process per GPU) with the v2
    optimiser, parts and a train loader that keeps the last, smaller batch (drop_last=False, :815).
"""
from __future__ import annotations

import pickle
import random
from pathlib import Path
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
import torch.utils.data

from . import train as _train
from .slowfast import init_my_slowfast

CHANNELS = ("R", "G", "B", "U", "V", "F0", "F1")     # frames_u8's last axis; slow = [0:5], fast = [5:7]


class PartCompose:
    """DensePose part ids and their compositions (new_feature_test.py:470-547), restated."""
    lHand = [4]
    rHand = [3]
    lUpArm = [15, 17]
    rUpArm = [16, 18]
    lLoArm = [19, 21]
    rLoArm = [20, 22]
    torso = [1, 2]
    head = [23, 24]
    lArm = lUpArm + lLoArm
    rArm = rUpArm + rLoArm
    TorsoArmHand = torso + lArm + rArm + lHand + rHand
    lHandLoArm = lHand + lLoArm
    lHandArm = lHand + lArm
    lHandArmTorso = lHand + lArm + torso
    rHandLoArm = rHand + rLoArm
    rHandArm = rHand + rArm
    rHandArmTorso = rHand + rArm + torso

    @staticmethod
    def combine_box_xyxy(box_arr) -> tuple:
        """(N, 4) boxes -> their union (min x1, min y1, max x2, max y2)"""
        assert len(box_arr) > 0
        a = np.array(box_arr)
        return (min(a[:, 0]), min(a[:, 1]), max(a[:, 2]), max(a[:, 3]))

    def combine_spatial_box_xyxy(self, part_boxes, part_list):
        """one frame's [P][4] part boxes -> the union over part_list (None parts skipped); None when no part is there"""
        if part_boxes is None:
            return None
        boxes = [part_boxes[p] for p in part_list]
        boxes = [b for b in boxes if b is not None]
        return self.combine_box_xyxy(np.array(boxes)) if boxes else None

    def combine_temporal_box_xyxy(self, temporal_part_boxes, part_list):
        """[T][P][4] -> the union over the frames (None frames and frames without any of the parts skipped)"""
        per_frame = [self.combine_spatial_box_xyxy(pb, part_list) for pb in temporal_part_boxes]
        per_frame = [b for b in per_frame if b is not None]
        if not per_frame:
            raise ValueError(f"no box of parts {list(part_list)} in any frame of the clip")
        return self.combine_box_xyxy(per_frame)


def parts_of(name: str) -> List[int]:
    """MODEL.PARTS -> the part ids (a PartCompose attribute name, e.g. 'lHandArmTorso')"""
    parts = getattr(PartCompose, str(name), None)
    if not isinstance(parts, list):
        raise ValueError(f"MODEL.PARTS={name!r} is not a PartCompose composition")
    return list(parts)


def random_sampling(seq_len: int, clip_len: int, rng=random) -> List[int]:
    """new_feature_test.py:663-669: a random start (randint, both ends included), indices wrapped mod seq_len"""
    start = rng.randint(0, max(0, seq_len - clip_len))
    return [i % seq_len for i in range(start, start + clip_len)]


def uniform_sampling(seq_len: int, clip_len: int, rng=random) -> List[List[int]]:
    """new_feature_test.py:671-680: non-overlapping windows range(0, seq_len - clip_len, clip_len); one random clip when
    the video is not longer than a clip"""
    if seq_len <= clip_len:
        return [random_sampling(seq_len, clip_len, rng)]
    return [list(range(t, t + clip_len)) for t in range(0, seq_len - clip_len, clip_len)]


def change_base(path: Path, base: str) -> Path:
    """ChaPath.change_base (new_feature_test.py:40-46): the 4th path component from the end -> base"""
    parts = list(Path(path).parts)
    parts[-4] = base
    return Path(*parts)


def decord_read_video(filename: Path, channels: int, frames: Sequence[int], format: str = "gray") -> torch.Tensor:
    """VideoIO.read_video_TCHW (new_feature_test.py:95-132): (T, C, H, W) uint8; 'rgb24' reads one colour video, 'gray'
    reads the channel videos '<c>_<name>' and keeps their first plane."""
    try:
        import decord
    except ImportError as e:
        raise RuntimeError("ChalearnGestureFrames needs decord to read videos (not installed); pass read_video=") from e
    decord.bridge.set_bridge("torch")
    if format == "rgb24":
        return decord.VideoReader(str(filename)).get_batch(list(frames)).permute(0, 3, 1, 2)
    planes = [decord.VideoReader(str(Path(filename.parent, f"{c}_{filename.name}"))).get_batch(list(frames))[..., 0]
              for c in range(channels)]
    return torch.stack(planes, dim=1)


class ChalearnGestureFrames(torch.utils.data.Dataset):
    """The reference's ChalearnGestureDataset (new_feature_test.py:556-710) with the crop and resize left to the device.

    labels: the reference's ``Labels(cfg).from_set(name_of_set)`` list of (rgb path, depth path, 1-based label).  Items:
    {'frames_u8': (T, H, W, 7) uint8 [R, G, B, U, V, F0, F1], 'box': int32 (x1, y1, x2, y2) clamped to the frame,
    'label': label - 1}; a list of them for sampling='uniform'.  read_video(path, channels, indices, format) -> (T, C, H, W)
    uint8 is injectable (default: decord, as the reference).  Under MODEL.AFFINE a random train clip also carries 'warp':
    (6,) float32, the row of ``input_pipeline.draw_affine`` on the resized S x S clip (``train.draw_crop_or_warp``)."""

    def __init__(self, cfg, name_of_set: str, parts, sampling: str, labels, read_video: Optional[Callable] = None):
        assert name_of_set in ("train", "test", "valid")
        assert sampling in ("random", "uniform")
        self.label_list = list(labels)
        self.parts = list(parts)
        self.clip_len = cfg.CHALEARN.CLIP_LEN
        self.root, self.sample_base = cfg.CHALEARN.ROOT, cfg.CHALEARN.SAMPLE
        self.box_base, self.flow_base, self.uv_base = cfg.CHALEARN.BOX, cfg.CHALEARN.FLOW_VIDEO, cfg.CHALEARN.UV_VIDEO
        self.sampling = sampling
        self.compose = PartCompose()
        self.read_video = read_video or decord_read_video
        self.rng = random
        # MODEL.COLOR_JITTER: the train set's random clips carry their ColorJitter draws (input_pipeline.draw_color_jitter)
        self.jitter = _train.jitter_ranges(cfg) if name_of_set == "train" else None
        # MODEL.AFFINE: they carry their warp row too, drawn before the jitter row
        self.affine_cfg = cfg if name_of_set == "train" and _train.affine_ranges(cfg) is not None else None

    def __len__(self):
        return len(self.label_list)

    def clip_box(self, boxes, clip_indices, h: int, w: int) -> torch.Tensor:
        """the union box of the clip's frames, x1, y1 = max(0, .) as the reference, x2, y2 clamped to the frame as its
        slice clamps them; an empty box is a ValueError"""
        x1, y1, x2, y2 = (int(v) for v in self.compose.combine_temporal_box_xyxy([boxes[i] for i in clip_indices], self.parts))
        x1, y1 = max(0, x1), max(0, y1)
        x2, y2 = min(x2, w), min(y2, h)
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"empty part box {(x1, y1, x2, y2)} in a {w}x{h} frame")
        return torch.tensor([x1, y1, x2, y2], dtype=torch.int32)

    def _features_from_indices(self, clip_indices, boxes, rgb_path, label):
        flow = self.read_video(change_base(rgb_path, self.flow_base), 2, clip_indices, "gray")
        uv = self.read_video(change_base(rgb_path, self.uv_base), 2, clip_indices, "gray")
        rgb = self.read_video(rgb_path, 0, clip_indices, "rgb24")
        x = torch.cat([rgb, uv, flow], dim=1)                          # T, 7, H, W
        _, _, h, w = x.shape
        box = self.clip_box(boxes, clip_indices, h, w)
        item = {"frames_u8": x.permute(0, 2, 3, 1).contiguous(), "box": box, "label": label - 1}
        if self.affine_cfg is not None and self.sampling == "random":
            item["warp"] = _train.draw_crop_or_warp(self.affine_cfg, int(self.affine_cfg.MODEL.INPUT_SIZE))[1]
        if self.jitter is not None and self.sampling == "random":
            from .input_pipeline import draw_color_jitter
            item["jitter"] = draw_color_jitter(1, *self.jitter)[0]
        return item

    def _rgb_path_and_boxes(self, index) -> tuple:
        rgb_path = Path(self.root, self.sample_base, self.label_list[index][0])
        with change_base(rgb_path, self.box_base).with_suffix(".pkl").open("rb") as f:
            return rgb_path, pickle.load(f)

    # ---- what input_pipeline.ResidentGestureSet reads the train set through (MODEL.RESIDENT_TRAIN)
    def seq_len(self, i: int) -> int:
        return len(self._rgb_path_and_boxes(i)[1]) - 1

    def label(self, i: int) -> int:
        return self.label_list[i][2] - 1

    def frame_boxes(self, i: int) -> torch.Tensor:
        """(seq_len, 4) int32: every frame's union box over the parts, ``NO_BOX`` where none is there; reads the box pickle only"""
        from .input_pipeline import NO_BOX
        _, boxes = self._rgb_path_and_boxes(i)
        rows = [self.compose.combine_spatial_box_xyxy(pb, self.parts) for pb in boxes[:len(boxes) - 1]]
        return torch.tensor([NO_BOX if b is None else [int(v) for v in b] for b in rows], dtype=torch.int32).reshape(-1, 4)

    def video_item(self, i: int, indices=None) -> dict:
        """{'frames_pool': (L, H, W, 7) uint8 of the frames at indices (default: all seq_len of them), 'windows': (1, L)}"""
        rgb_path, boxes = self._rgb_path_and_boxes(i)
        indices = list(range(len(boxes) - 1)) if indices is None else list(indices)
        flow = self.read_video(change_base(rgb_path, self.flow_base), 2, indices, "gray")
        uv = self.read_video(change_base(rgb_path, self.uv_base), 2, indices, "gray")
        rgb = self.read_video(rgb_path, 0, indices, "rgb24")
        x = torch.cat([rgb, uv, flow], dim=1).permute(0, 2, 3, 1).contiguous()
        return {"frames_pool": x, "windows": torch.arange(len(indices), dtype=torch.int32)[None]}

    def __getitem__(self, index):
        label = self.label_list[index][2]
        rgb_path, boxes = self._rgb_path_and_boxes(index)
        seq_len = len(boxes) - 1                    # as the reference: the reader's frame count is one short
        if self.sampling == "random":
            return self._features_from_indices(random_sampling(seq_len, self.clip_len, self.rng), boxes, rgb_path, label)
        return [self._features_from_indices(ci, boxes, rgb_path, label)
                for ci in uniform_sampling(seq_len, self.clip_len, self.rng)]


class SyntheticGesture(torch.utils.data.Dataset):
    """Seeded stand-in with ChalearnGestureFrames' item contract: random uint8 frames of h x w with a random box per clip
    (train -> dict, test -> list of dicts), for tests and tools/bench_v2.py.
    videos=True (train only): every video is ONE fixed run of frames_per_video = (lo, hi) seeded frames with a seeded
    per-frame box table (every no_box_every-th frame has none: a ``NO_BOX`` row), a train item is a random clip of it, and
    the set offers what ``input_pipeline.ResidentGestureSet`` reads a train set through -- seq_len, label, video_item and
    frame_boxes.  The default construction does not offer them."""

    def __init__(self, cfg, name_of_set: str, num_videos: int = 8, clips_per_video=(1, 3), seed: int = 0,
                 h: int = 240, w: int = 320, min_box: int = 15, videos: bool = False, frames_per_video=None,
                 no_box_every: int = 5):
        self.cfg, self.name = cfg, name_of_set
        self.t, self.h, self.w, self.min_box = int(cfg.CHALEARN.CLIP_LEN), h, w, min_box
        g = torch.Generator().manual_seed(seed)
        self.labels = torch.randint(0, cfg.CHALEARN.NUM_CLASS, (num_videos,), generator=g).tolist()
        self.nclips = torch.randint(clips_per_video[0], clips_per_video[1] + 1, (num_videos,), generator=g).tolist()
        self.seed = seed
        self.videos = bool(videos)
        if self.videos:
            assert name_of_set == "train", "SyntheticGesture(videos=True) is a train set"
            lo, hi = frames_per_video or (max(2, self.t // 2), 3 * self.t)
            gv = torch.Generator().manual_seed(seed * 86028121 + 5)             # its own draws: the default mode's stay as they are
            self.vframes = torch.randint(lo, hi + 1, (num_videos,), generator=gv).tolist()
            self.no_box_every, self.rng = int(no_box_every), random
            self.seq_len, self.label, self.video_item, self.frame_boxes = (self._seq_len, self._label, self._video_item,
                                                                           self._frame_boxes)

    def __len__(self):
        return len(self.labels)

    # ---- videos=True: the resident contract
    def _seq_len(self, i: int) -> int:
        return self.vframes[i]

    def _label(self, i: int) -> int:
        return self.labels[i]

    def _video_frame(self, i: int, k: int) -> torch.Tensor:
        g = torch.Generator().manual_seed((self.seed * 7919 + i) * 100003 + k)
        return torch.randint(0, 256, (self.h, self.w, 7), generator=g, dtype=torch.uint8)

    def _frame_boxes(self, i: int) -> torch.Tensor:
        """frame 0 always has a box; every no_box_every-th frame after it has none"""
        from .input_pipeline import NO_BOX
        g = torch.Generator().manual_seed(self.seed * 6007 + i * 17 + 1)
        rows = []
        for k in range(self.vframes[i]):
            x1 = int(torch.randint(0, self.w - self.min_box, (1,), generator=g))
            y1 = int(torch.randint(0, self.h - self.min_box, (1,), generator=g))
            x2 = int(torch.randint(x1 + self.min_box, self.w + 1, (1,), generator=g))
            y2 = int(torch.randint(y1 + self.min_box, self.h + 1, (1,), generator=g))
            rows.append(NO_BOX if k and self.no_box_every and k % self.no_box_every == 0 else (x1, y1, x2, y2))
        return torch.tensor(rows, dtype=torch.int32)

    def _video_item(self, i: int, indices=None) -> dict:
        indices = list(range(self.vframes[i])) if indices is None else list(indices)
        return {"frames_pool": torch.stack([self._video_frame(i, k) for k in indices]),
                "windows": torch.arange(len(indices), dtype=torch.int32)[None]}

    def _video_clip(self, i: int) -> dict:
        """a train item of the loader path: a random clip of video i, its frames' union box"""
        idx = random_sampling(self.vframes[i], self.t, self.rng)
        b = self._frame_boxes(i)[idx]
        box = torch.stack([b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()])
        item = {"frames_u8": self._video_item(i, idx)["frames_pool"], "box": box, "label": self.labels[i]}
        if _train.affine_ranges(self.cfg) is not None:           # MODEL.AFFINE: the warp row, drawn before the jitter row
            item["warp"] = _train.draw_crop_or_warp(self.cfg, int(self.cfg.MODEL.INPUT_SIZE))[1]
        ranges = _train.jitter_ranges(self.cfg)
        if ranges is not None:
            from .input_pipeline import draw_color_jitter
            item["jitter"] = draw_color_jitter(1, *ranges)[0]
        return item

    def _clip(self, i, j):
        g = torch.Generator().manual_seed(self.seed * 7919 + i * 31 + j)
        frames = torch.randint(0, 256, (self.t, self.h, self.w, 7), generator=g, dtype=torch.uint8)
        x1 = int(torch.randint(0, self.w - self.min_box, (1,), generator=g))
        y1 = int(torch.randint(0, self.h - self.min_box, (1,), generator=g))
        x2 = int(torch.randint(x1 + self.min_box, self.w + 1, (1,), generator=g))
        y2 = int(torch.randint(y1 + self.min_box, self.h + 1, (1,), generator=g))
        item = {"frames_u8": frames, "box": torch.tensor([x1, y1, x2, y2], dtype=torch.int32), "label": self.labels[i]}
        if self.name == "train" and _train.affine_ranges(self.cfg) is not None:
            item["warp"] = _train.draw_crop_or_warp(self.cfg, int(self.cfg.MODEL.INPUT_SIZE), generator=g)[1]
        ranges = _train.jitter_ranges(self.cfg) if self.name == "train" else None
        if ranges is not None:
            from .input_pipeline import draw_color_jitter
            item["jitter"] = draw_color_jitter(1, *ranges, generator=g)[0]
        return item

    def __getitem__(self, i):
        if self.videos:
            return self._video_clip(i)
        if self.name == "train":
            return self._clip(i, 0)
        return [self._clip(i, j) for j in range(self.nclips[i])]


class ModelManager(_train.ModelManager):
    """new_feature_test.py:712-775: init_my_slowfast(cfg, (5, 2), (64, 8)) with the v1 pretrained surgery, and
    prepare_data for the reference's float batch or the uint8 batch of ChalearnGestureFrames."""

    def __init__(self, cfg, device="cuda", backend=None):
        self.cfg, self.device, self.backend = cfg, device, backend
        self._pre = None
        self._lut = None
        self._roi = None
        self._jit = None
        self._mix = None
        self.train_affine = False                        # Trainer.train_epoch under MODEL.AFFINE: a float TRAIN batch is refused
        self.arch = "ref"
        self.init_model = self._init_v2_model
        self.prepare_data = self._prepare_v2_data

    def _init_v2_model(self):
        model = init_my_slowfast(self.cfg, (5, 2), (64, 8), device=self.device, backend=self.backend)
        ckpt = Path("pretrained", "SLOWFAST_8x8_R50.pyth")          # :741-759 (absent offline: random init)
        if ckpt.is_file():
            state = torch.load(ckpt, map_location="cpu", weights_only=True)["model_state"]
            self.load_pretrained(model, self.delete_mismatch(state))
        else:
            print(f"warning: {ckpt} not found, training from the reference init scheme")
        return model

    def mix_channels(self) -> int:
        return 7                                         # R, G, B, U, V and the two flow channels: the model reads them all

    def roi_resize(self) -> "RoiResize":
        if self._roi is None:
            from .input_pipeline import RoiResize
            from .slowfast import _DTYPES
            dtype = _DTYPES[str(self.cfg.MODEL.get("DTYPE", "fp32")).lower()]
            self._roi = RoiResize(int(self.cfg.MODEL.INPUT_SIZE), self.device, self.backend, out_dtype=dtype,
                                  antialias=bool(self.cfg.MODEL.get("RESIZE_ANTIALIAS", True)))
        return self._roi

    def _prepare_v2_data(self, batch):
        """-> [slow (N, 5, T, S, S), fast (N, 2, T, S, S)], labels.  The uint8 batch {'frames_u8', 'box'[, 'crop' | 'warp']} is
        resized on the device into one (N, T, 7, S, S) tensor whose channel slices are the two pathways (no copy) -- with
        'warp' (MODEL.AFFINE) the resize is sampled through each clip's matrix in that same single launch
        (include/sfk_roi_warp.h), then jittered, then mixed; the float batch with 'warp' is refused: it has no uint8 frames; a
        'clip_v2' batch (input_pipeline.ResidentGestureSet, MODEL.RESIDENT_TRAIN) already is that tensor; the
        float batch {'rgb', 'uv', 'flow'} is the reference's permute + cat (:761-769).  An optional 'jitter' (N, 8) entry
        (input_pipeline.draw_color_jitter) applies ColorJitter to the R, G, B planes on the device: after the resize and
        the crop of a uint8 batch ("Optional Augment (crop&pad, color jitter)", :608-611), to the device copy of 'rgb' of
        a float batch; the values are image values in [0, 1] (mean 0, std 1).  An optional 'mix' entry (the device table of
        input_pipeline.ClipMix.load) then mixes the finished float clip with its partner clip (_mix_clip)."""
        y = self._h2d(batch["label"])
        if "clip_v2" in batch or "frames_u8" in batch:
            x = (batch["clip_v2"] if "clip_v2" in batch else
                 self.roi_resize()(batch["frames_u8"], batch["box"], batch.get("crop"), warp=batch.get("warp")))
            if "jitter" in batch:
                self.color_jitter()(x, batch["jitter"])
            x = self._mix_clip(x, batch)
            x = torch.permute(x, [0, 2, 1, 3, 4])
            return [x[:, 0:5], x[:, 5:7]], y
        if "warp" in batch or self.train_affine:
            raise ValueError("the float batch {'rgb', 'uv', 'flow'} is already resized on the host: there are no uint8 frames for "
                             "the device-side affine sampling (MODEL.AFFINE) to read; feed 'frames_u8' and 'box', use "
                             "MODEL.RESIDENT_TRAIN, or turn MODEL.AFFINE off")
        rgb, uv, flow = (self._h2d(batch[k]) for k in ("rgb", "uv", "flow"))
        if "jitter" in batch:
            rgb = self.color_jitter()(self._own(rgb, batch["rgb"]), batch["jitter"])
        rgb, uv, flow = (torch.permute(t, [0, 2, 1, 3, 4]) for t in (rgb, uv, flow))
        slow = torch.cat([rgb, uv], dim=1)
        if "mix" in batch:                               # the float batch: one launch per pathway tensor, through their (N,T,C,S,S) views
            flow = flow.contiguous()                     # (the permuted view is the loader's own memory on a device batch)
            for x in (slow, flow):
                self._mix_clip(torch.permute(x, [0, 2, 1, 3, 4]), batch)
        return [slow, flow], y


class Trainer(_train.Trainer):
    """new_feature_test.py:796-979 on train.Trainer: SGD(lr, momentum 0.9), MODEL.PARTS, a train loader that keeps the
    last smaller batch, uniform non-overlapping test windows; checkpoints, eval and the multi-process path as train.Trainer."""
    train_drop_last = False                              # :815
    momentum = 0.9                                       # :832
    pool_stem_unsupported = ("the v2 part-box route resizes the box crop BEFORE the stem, so its stems read that resized float "
                             "clip and not the pool's frames")
    resident_methods_missing = ("seq_len(i), label(i), video_item(i, indices=None) and frame_boxes(i), which ResidentGestureSet "
                                "needs to gather RoiResize's uncropped 240 x 320 x 7 frames and their boxes from a frame pool "
                                "(ChalearnGestureFrames and SyntheticGesture(videos=True) do)")

    def _model_manager(self, cfg, device, backend):
        return ModelManager(cfg, device=device, backend=backend)

    def _make_step(self, eng, use_graph, reducer):
        kw = self._optim_kwargs()
        if kw.get("decay_mode") == "decoupled":
            raise ValueError("MODEL.WEIGHT_DECAY_MODE: decoupled needs Adam; the v2 trainer runs SGD (torch has no decoupled "
                             "SGD): set WEIGHT_DECAY_MODE: l2")
        return _train.TrainStep(eng, lr=self.cfg.MODEL.LR, use_graph=use_graph, reducer=reducer, optimizer="sgd",
                                momentum=self.momentum, **kw, **self._mix_kwargs(), **self._ema_kwargs(), **self._group_kwargs())

    def mix_frame(self) -> int:
        return int(self.cfg.MODEL.INPUT_SIZE)

    def train_epoch(self):
        """MODEL.AFFINE: the train batches must be ones the device can sample (uint8 frames or the resident set); evaluation
        is unchanged"""
        self.mm.train_affine = _train.affine_ranges(self.cfg) is not None
        try:
            return super().train_epoch()
        finally:
            self.mm.train_affine = False

    def _offers_resident(self, train_set) -> bool:
        from .input_pipeline import GESTURE_METHODS, offers_resident
        return offers_resident(train_set, GESTURE_METHODS)

    def _build_resident(self, train_set, backend):
        """MODEL.RESIDENT_TRAIN: the frames stay on the device, whole (a batch is one sfk_roi_resize_pool launch) or, with
        MODEL.RESIDENT_STORE: box, cropped to what their video's clips can read (one sfk_roi_resize_ragged launch)"""
        from .input_pipeline import ResidentGestureSet
        return ResidentGestureSet(train_set, self.cfg, self.device, backend, batch_size=self.batch_size,
                                  drop_last=self.train_drop_last, num_workers=self.num_workers,
                                  jitter=_train.jitter_ranges(self.cfg),
                                  store=str(self.cfg.MODEL.get("RESIDENT_STORE", "frame")),
                                  affine=_train.affine_ranges(self.cfg))

    def _reference_datasets(self):
        try:
            from utils.chalearn import Labels                       # the reference's label lists, unchanged
        except Exception as e:
            raise RuntimeError("no datasets / loaders were given and the reference's utils.chalearn is not importable here "
                               f"({e}); pass train_set/test_set (e.g. SyntheticGesture)") from e
        parts = parts_of(self.cfg.MODEL.get("PARTS", "lHandArmTorso"))
        return (ChalearnGestureFrames(self.cfg, "train", parts, "random", Labels(self.cfg).from_set("train")),
                ChalearnGestureFrames(self.cfg, "test", parts, "uniform", Labels(self.cfg).from_set("test")))
