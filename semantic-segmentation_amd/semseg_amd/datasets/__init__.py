"""Integer-exact pieces of the input pipeline that sit next to the hot path
(SURVEY.md section 8a rows S1, S2): the rank-sharding sampler and the
nearest-neighbour label resize."""
from .sampler import DistributedSampler, shard_indices      # noqa: F401
from .transforms import nearest_index_table, resize_labels_nearest   # noqa: F401
from .transforms import (ColorJitter, JitterParams, adjust_brightness, adjust_contrast, adjust_hue,   # noqa: F401
                         adjust_saturation, color_jitter, crop_flip_normalize)
from .transforms import BlurParams, RandomGaussianBlur, gaussian_blur, gaussian_taps   # noqa: F401
from .transforms import AugmentParams, RandAugment, rand_augment   # noqa: F401
from .transforms import CropPlan, RandomSizeAndCrop, pad_u8, resize_image_bicubic   # noqa: F401
from .uniform import (build_centroids, build_epoch, calc_tile_locations, class_centroids, class_centroids_all,   # noqa: F401
                      class_centroids_image, pooled_class_centroids_all, random_sampling)
from .autolabel import label_plan, label_steps, prepare_labels, prob_cut, read_labels   # noqa: F401
