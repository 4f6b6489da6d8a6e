"""Configuration read by the hot path.

In drop-in mode (under the reference's train.py) `sync_from_reference()` copies
the values the reference's global `cfg` (config.py:60-190) holds for these
fields after `assert_and_infer_cfg`; standalone (bench.py, tests) the defaults
below are the reference's defaults for the HRNet-OCR-MScale recipes.
"""


class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def _defaults():
    c = AttrDict()
    c.MODEL = AttrDict(
        BNFUNC=None,                 # config.py:216-225 picks the norm layer; None -> semseg_amd.nn.BatchNorm2d
        ALIGN_CORNERS=False,         # config.py:125
        MSCALE=False,                # config.py:122; assert_and_infer_cfg sets it for the mscale / attnscale architectures
        MSCALE_LO_SCALE=0.5,         # config.py:126
        N_SCALES=None,               # config.py:124
        SEGATTN_BOT_CH=256,          # config.py:130
        ASPP_BOT_CH=256,             # config.py:131
        MSCALE_INNER_3x3=True,       # config.py:131
        HRNET_CHECKPOINT="",         # config.py:147 (empty: random init, no file needed)
        WRN38_CHECKPOINT="",         # config.py:145 (empty: random init; else network/wider_resnet.py:405-409)
        X71_CHECKPOINT="",           # config.py:145-146 (empty: random init; else network/xception.py:270-279)
        SRNX_CHECKPOINT="",          # (empty: random init; else a LOCAL file, network/seresnext.py -- the reference downloads)
        OCR=AttrDict(MID_CHANNELS=512, KEY_CHANNELS=256),   # config.py:157-158
        # cfg.MODEL.OCR_EXTRA, config.py:161-190 (HRNetV2-W48)
        OCR_EXTRA=AttrDict(
            STAGE1=AttrDict(NUM_MODULES=1, NUM_BLOCKS=[4], NUM_CHANNELS=[64], BLOCK="BOTTLENECK"),
            STAGE2=AttrDict(NUM_MODULES=1, NUM_BRANCHES=2, NUM_BLOCKS=[4, 4], NUM_CHANNELS=[48, 96], BLOCK="BASIC"),
            STAGE3=AttrDict(NUM_MODULES=4, NUM_BRANCHES=3, NUM_BLOCKS=[4, 4, 4], NUM_CHANNELS=[48, 96, 192], BLOCK="BASIC"),
            STAGE4=AttrDict(NUM_MODULES=3, NUM_BRANCHES=4, NUM_BLOCKS=[4, 4, 4, 4], NUM_CHANNELS=[48, 96, 192, 384], BLOCK="BASIC"),
        ),
    )
    c.LOSS = AttrDict(OCR_ALPHA=0.4, OCR_AUX_RMI=False, SUPERVISED_MSCALE_WT=0)   # config.py:150-155
    c.DATASET = AttrDict(
        NUM_CLASSES=19, IGNORE_LABEL=255,
        NAME="",                     # config.py:98 (assert_and_infer_cfg: args.dataset, config.py:244)
        CLASS_UNIFORM_PCT=0.5,       # config.py:102 (--class_uniform_pct, train.py:78): share of class-uniform items per epoch
        CLASS_UNIFORM_TILE=1024,     # config.py:103 (--class_uniform_tile): names the centroid cache (datasets/uniform.py)
        CLASS_UNIFORM_BIAS=None,     # config.py:253: per-class multipliers of the per-class item count, or None
        CENTROID_ROOT="/home/dcg-adlr-atao-data.cosmos277/assets/uniform_centroids",   # config.py:52, 82-83
        TRANSLATE_AUG_FIX=False,     # config.py:112 (--translate_aug_fix, config.py:266-267)
        MEAN=[0.485, 0.456, 0.406],  # config.py:96-97: what ImageDumper de-normalises with (utils/dumper.py)
        STD=[0.229, 0.224, 0.225],
        # the auto-labelled coarse data path (datasets/autolabel.py; base_loader.py:152-229, uniform.py:104-121)
        CITYSCAPES_DIR="/home/dcg-adlr-atao-data.cosmos277/assets/data/Cityscapes",                     # config.py:78-79
        CITYSCAPES_CUSTOMCOARSE="/home/dcg-adlr-atao-data.cosmos277/assets/data/Cityscapes/autolabelled",   # config.py:80-81
        COARSE_BOOST_CLASSES=None,   # config.py:104, 249-251 (--coarse_boost_classes): cityscapes.py's file discovery reads it
        CUSTOM_COARSE_PROB=None,     # config.py:107, 234-235 (--custom_coarse_prob): labels below this confidence are ignored
        MASK_OUT_CITYSCAPES=False,   # config.py:108, 300-301 (--mask_out_cityscapes): the drop mask of auto-labelled items
    )
    c.DATASET_INST = None            # config.py:381 (update_dataset_inst): colorize_mask / id_to_trainid of ImageDumper
    c.RESULT_DIR = None              # config.py:64, 298 (args.result_dir): where ImageDumper writes
    c.GLOBAL_RANK = 0                # config.py:49, 358: only rank 0 dumps images
    c.OPTIONS = AttrDict(INIT_DECODER=False)
    c.EPOCH = 0                      # config.py:50 (train.py sets it every epoch)
    c.BATCH_WEIGHTING = False        # config.py:55 (class weights over the batch instead of per image)
    c.BORDER_WINDOW = 1              # config.py:58 (half width of the label relaxation window)
    c.REDUCE_BORDER_EPOCH = -1       # config.py:60 (the 'scl-poly' LR schedule switches there)
    c.STRICTBORDERCLASS = None       # config.py:62 (classes whose pixels are never relaxed)
    c.DROPOUT_COARSE_BOOST_CLASSES = None   # config.py:350-353 (--custom_coarse_dropout_classes): datasets/autolabel.py
    return c


cfg = _defaults()


def sync_from_reference(ref_cfg):
    """Copy the fields the hot path reads from the reference's global cfg."""
    m = ref_cfg.MODEL
    for k in ("ALIGN_CORNERS", "MSCALE", "MSCALE_LO_SCALE", "N_SCALES", "SEGATTN_BOT_CH", "ASPP_BOT_CH", "MSCALE_INNER_3x3",
              "HRNET_CHECKPOINT", "WRN38_CHECKPOINT", "X71_CHECKPOINT", "SRNX_CHECKPOINT"):
        if hasattr(m, k):
            cfg.MODEL[k] = getattr(m, k)
    cfg.MODEL.OCR.MID_CHANNELS = m.OCR.MID_CHANNELS
    cfg.MODEL.OCR.KEY_CHANNELS = m.OCR.KEY_CHANNELS
    for k in ("OCR_ALPHA", "OCR_AUX_RMI", "SUPERVISED_MSCALE_WT"):
        cfg.LOSS[k] = getattr(ref_cfg.LOSS, k)
    cfg.DATASET.NUM_CLASSES = ref_cfg.DATASET.NUM_CLASSES
    cfg.DATASET.IGNORE_LABEL = ref_cfg.DATASET.IGNORE_LABEL
    for k in ("DATASET_INST", "RESULT_DIR", "GLOBAL_RANK"):
        if hasattr(ref_cfg, k):
            cfg[k] = getattr(ref_cfg, k)
    for k in ("NAME", "CLASS_UNIFORM_PCT", "CLASS_UNIFORM_TILE", "CLASS_UNIFORM_BIAS", "CENTROID_ROOT", "TRANSLATE_AUG_FIX",
              "MEAN", "STD", "CITYSCAPES_DIR", "CITYSCAPES_CUSTOMCOARSE", "COARSE_BOOST_CLASSES", "CUSTOM_COARSE_PROB",
              "MASK_OUT_CITYSCAPES"):
        if hasattr(ref_cfg.DATASET, k):         # (CLASS_UNIFORM_BIAS exists only after assert_and_infer_cfg)
            cfg.DATASET[k] = getattr(ref_cfg.DATASET, k)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = getattr(ref_cfg, "DROPOUT_COARSE_BOOST_CLASSES", None)
    cfg.OPTIONS.INIT_DECODER = ref_cfg.OPTIONS.INIT_DECODER
    cfg.REDUCE_BORDER_EPOCH = getattr(ref_cfg, "REDUCE_BORDER_EPOCH", -1)
    cfg.EPOCH = getattr(ref_cfg, "EPOCH", 0)
    cfg.BATCH_WEIGHTING = getattr(ref_cfg, "BATCH_WEIGHTING", False)
    cfg.BORDER_WINDOW = getattr(ref_cfg, "BORDER_WINDOW", 1)
    cfg.STRICTBORDERCLASS = getattr(ref_cfg, "STRICTBORDERCLASS", None)
    for k in ("MSCALE_OLDARCH", "MSCALE_DROPOUT", "MSCALE_CAT_SCALE_FLT"):      # config.py:132-135
        assert not getattr(m, k, False), "cfg.MODEL.%s is not on the accelerated path" % k
