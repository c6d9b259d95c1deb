"""Config surface of the reference, drop-in: same keys, same defaults, same merge order.

Mirrors /root/reference/config/defaults.py:4-60 (yacs CfgNode tree, get_cfg, get_override_cfg) and
/root/reference/config/crop_cfg.py:22-57 (crop folder -> pixel size).  yacs is not installed in this image, so
``CfgNode`` is a small compatible subset: attribute access, clone(), merge_from_file(yaml), merge_from_list().
New keys (MODEL.DTYPE, MODEL.ARCH, MODEL.DEPTH, DIST.*) default to the reference's behaviour (fp32, its own geometry, 1 process).
"""
from __future__ import annotations

import copy
from pathlib import Path

import yaml


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self) -> "CfgNode":
        return copy.deepcopy(self)

    def _merge(self, other: dict, path=""):
        for k, v in other.items():
            if k not in self:
                raise KeyError(f"Non-existent config key: {path}{k}")
            if isinstance(self[k], CfgNode):
                if not isinstance(v, dict):
                    raise ValueError(f"{path}{k} must be a mapping")
                self[k]._merge(v, f"{path}{k}.")
            else:
                old = self[k]
                if isinstance(old, float) and isinstance(v, str):
                    v = float(v)          # PyYAML reads '2e-4' as a string; yacs casts it back
                if isinstance(old, float) and isinstance(v, int) and not isinstance(v, bool):
                    v = float(v)
                if old is not None and v is not None and type(old) is not type(v):
                    raise ValueError(f"Type mismatch for {path}{k}: {type(old).__name__} vs {type(v).__name__}")
                self[k] = v

    def merge_from_file(self, path) -> None:
        with open(str(path), "r") as f:
            data = yaml.safe_load(f) or {}
        self._merge(data)

    def merge_from_list(self, kv) -> None:
        assert len(kv) % 2 == 0
        for k, v in zip(kv[0::2], kv[1::2]):
            node = self
            parts = k.split(".")
            for p in parts[:-1]:
                node = node[p]
            node._merge({parts[-1]: v}, ".".join(parts[:-1]) + ("." if len(parts) > 1 else ""))


_C = CfgNode()
_C.CHALEARN = CfgNode()
_C.DEBUG = False
_C.CHALEARN.ROOT = '/media/zc/C2000Pro-1TB/ChaLearnIsoAllClass'
_C.CHALEARN.NUM_CLASS = 249
_C.CHALEARN.BATCH_SIZE = 10
_C.CHALEARN.ISO = '0_Iso'
_C.CHALEARN.SAMPLE = '1_Sample'
_C.CHALEARN.SAMPLE_CLASS = 249
_C.CHALEARN.IMG = '2_Images'
_C.CHALEARN.IMG_SAMPLE_INTERVAL = 5
_C.CHALEARN.PAD = '3_Pad'
_C.CHALEARN.IUV = '4_IUV'
_C.CHALEARN.CSE = '4_CSE'
_C.CHALEARN.CROP_BODY = 'CropBody'
_C.CHALEARN.CLIP_LEN = 20
_C.CHALEARN.FLOW = '2_Flow'
_C.CHALEARN.FLOW_NPY = '2_Flow_npy'
_C.CHALEARN.IMG_ENERGY = '2_Images_energy'
_C.CHALEARN.FLOW_VIDEO = '2_Flow_New'
_C.CHALEARN.IUV_NEW = '4_IUV_New'
_C.CHALEARN.UV_VIDEO = '5_UV_Video'
_C.CHALEARN.BOX = '6_Box'
_C.DENSEPOSE = './detectron2/projects/DensePose'
_C.MODEL = CfgNode()
_C.MODEL.LOGS = 'logs'
_C.MODEL.NAME = 'new_feature_test'
_C.MODEL.CKPT_DIR = 'checkpoints'
_C.MODEL.R3D_INPUT = 'CropHTAH'
_C.MODEL.LR = 5e-4
_C.MODEL.FUSE = True
_C.MODEL.MAX_EPOCH = 100
_C.MODEL.INPUT_SIZE = 192
_C.NUM_CPU = 18
# ---- keys added by this engine; defaults reproduce the reference
_C.MODEL.DTYPE = 'fp32'        # 'fp32' (reference precision) | 'bf16' (benchmark precision)
_C.MODEL.ARCH = 'ref'          # 'ref' = init_my_slowfast geometry | 'canonical8x8' = SlowFast-R50 8x8 (BGR frames, PackPathway alpha 4)
_C.MODEL.DEPTH = 50            # the reference hard-codes 50 (model/my_slowfast.py:98); 18 / 26 = the small test networks
_C.MODEL.RES2D_BACKEND = 'torch'  # MODEL.NAME res2d: 'torch' (res2d.py, PyTorch kernels, fp32) | 'engine' (libsfk, MODEL.DTYPE)
_C.MODEL.PARTS = 'lHandArmTorso'  # gesture_v2 (new_feature_test.py:812): the PartCompose composition whose box each clip crops
_C.MODEL.RESIZE_ANTIALIAS = True  # gesture_v2: antialiased resize of the crop (torchvision >= 0.17 tensor Resize) or not (older)
_C.MODEL.POOL_STEM = False     # pooled routes (RESIDENT_TRAIN batches, pooled run_eval): the uint8 stems read the frame pool through its index table (True, include/sfk_u8stem_pool.h) or the gather writes the float clip first (False); it acts only on pooled routes that are in use -- without RESIDENT_TRAIN and without pooled test items it changes nothing
_C.MODEL.U8_STEM = False       # uint8 batches (<R3D_INPUT>_u8): the engine's stems read the frames (True) or DevicePreprocess writes the float clip first (False)
_C.MODEL.COLOR_JITTER = False  # train items carry the draws of torchvision's ColorJitter; applied on the device (include/sfk_aug.h)
_C.MODEL.JITTER_BRIGHTNESS = 0.5   # dataset/chalearn_dataset.py:49: ColorJitter(brightness=0.5, hue=0.1, contrast=0.3, saturation=0.2)
_C.MODEL.JITTER_CONTRAST = 0.3
_C.MODEL.JITTER_SATURATION = 0.2
_C.MODEL.JITTER_HUE = 0.1
_C.MODEL.AFFINE = False            # train clips are sampled through a random affine matrix per clip ON the device (include/sfk_warp.h) instead of RandomCrop's integer shift; the translation is still RandomCrop's draw
_C.MODEL.AFFINE_DEGREES = 10.0     # rotation, uniform in [-deg, deg] (input_pipeline.draw_affine)
_C.MODEL.AFFINE_SCALE = (0.85, 1.15)   # isotropic scale, uniform in [lo, hi]
_C.MODEL.AFFINE_SHEAR = 0.0        # x shear, degrees, uniform in [-shear, shear]
_C.MODEL.AFFINE_FLIP = 0.0         # probability of a horizontal flip; 0 because left and right hands differ
_C.MODEL.LABEL_SMOOTHING = 0.0    # the loss's smoothing mass eps: target (1 - eps) t + eps / K (include/sfk_mix.h); 0: sfk_softmax_ce as ever
_C.MODEL.MIXUP_ALPHA = 0.0         # > 0: Mixup with lam ~ Beta(alpha, alpha) on the device float clip, pairs i <-> N-1-i (input_pipeline.draw_mix)
_C.MODEL.CUTMIX_ALPHA = 0.0        # > 0: CutMix, the partner's box pasted; both > 0: CutMix with probability MIX_SWITCH_PROB
_C.MODEL.MIX_PROB = 1.0            # the probability that a pair is mixed at all
_C.MODEL.MIX_SWITCH_PROB = 0.5
_C.MODEL.MIX_SEED = 0              # the draws come from a generator seeded by (MIX_SEED, epoch, rank), in the main process
_C.MODEL.EMA_DECAY = 0.0           # > 0: keep an exponential moving average of the weights and BatchNorm statistics on the device (include/sfk_ema.h); 0: nothing is built
_C.MODEL.EMA_WARMUP = False        # the rate of step t is min(EMA_DECAY, (1 + t) / (10 + t)) (timm's ModelEmaV2)
_C.MODEL.EMA_EVAL = 'ema'          # what train() evaluates and saves with EMA on: 'ema' | 'live' | 'both' (both accuracies printed; the averaged model selects and is saved)
_C.MODEL.RESIDENT_TRAIN = False  # keep the decoded train frames on the device and gather the cropped clips there (input_pipeline.ResidentTrainSet)
_C.MODEL.RESIDENT_GB = 32.0     # RESIDENT_TRAIN: the size of the frame arena, GiB (its last BATCH_SIZE * CLIP_LEN slots are the spill region)
_C.MODEL.RESIDENT_STORE = 'frame'  # v2 RESIDENT_TRAIN: 'frame' keeps whole frames in a FramePool, 'box' only each video's part-box rectangle in a BoxArena of RESIDENT_GB bytes
# ---- the scheduled optimizer step (include/sfk_optim.h, schedule.py); every default keeps the plain sfk_adam / sfk_sgd launch
_C.MODEL.LR_SCHEDULE = 'constant'   # 'constant' | 'cosine' (linear warm-up, then cosine annealing to LR_MIN) | 'multistep'
_C.MODEL.LR_WARMUP_STEPS = 0        # cosine: optimizer steps of linear warm-up from LR / steps to LR
_C.MODEL.LR_MIN = 0.0               # cosine: the rate the annealing ends at
_C.MODEL.LR_MILESTONES = []         # multistep: the epochs at which the rate is multiplied by LR_GAMMA
_C.MODEL.LR_GAMMA = 0.1
_C.MODEL.WEIGHT_DECAY = 0.0
_C.MODEL.WEIGHT_DECAY_MODE = 'decoupled'   # 'decoupled' (AdamW; Adam only) | 'l2' (torch's Adam / SGD weight_decay)
_C.MODEL.WEIGHT_DECAY_SCOPE = 'weights'    # 'weights' (conv filters and the FC weight) | 'all' (biases and BatchNorm too)
_C.MODEL.CLIP_GRAD_NORM = 0.0       # clip_grad_norm_(max_norm) before the optimizer launch; 0 = off
# ---- parameter groups and frozen layers (include/sfk_groups.h, schedule.group_kwargs); both empty keeps the launches above
_C.MODEL.PARAM_GROUPS = []          # [selector, lr_mult] or [selector, lr_mult, wd_mult] in priority order; a selector is a state_dict() key prefix ('blocks.1.'), '@fresh' or '@pretrained' (what load_pretrained left untouched / filled)
_C.MODEL.FREEZE = []                # selectors of the tensors that do not train (freeze beats groups); eager steps only
_C.DIST = CfgNode()
_C.DIST.BUCKET_MB = 32         # gradient all-reduce bucket size


def get_cfg() -> CfgNode:
    """A copy of the defaults (reference config/defaults.py:50-54)."""
    return _C.clone()


def get_override_cfg() -> CfgNode:
    """Defaults + ../cfg_override.yaml when present (reference config/defaults.py:56-61)."""
    cfg = get_cfg()
    override = Path('..', 'cfg_override.yaml')
    if override.is_file():
        cfg.merge_from_file(override)
    return cfg


# crop folder -> square size in pixels (reference config/crop_cfg.py:18-55)
crop_resize_dict = {'CropHTAH': 192, 'CropLHand': 64, 'CropRHand': 64, 'CropLHandArm': 128, 'CropRHandArm': 128,
                    'CropTorso': 128}
crop_folder_list = list(crop_resize_dict.keys())
