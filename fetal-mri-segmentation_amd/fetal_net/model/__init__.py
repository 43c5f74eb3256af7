"""Builders looked up by name: `getattr(fetal_net.model, config['model_name'])` (reference fetal/train_fetal.py:32,
fetal_net/model/__init__.py:3-18).  The hot-path builders of SURVEY.md §8a: both U-Nets and both Isensee networks;
§8f row 4: the PatchGAN discriminators of the adversarial experiments; `norm_net_model`: an Isensee network with a linear output trained
through a frozen segmenter (the one consumer of the driver's `old_model_path`).  The optimizer classes the builders' `optimizer=`
keyword and `model.compile` take (fetal_net.optimizers) are at hand here too."""
from .unet3d.unet import unet_model_3d
from .unet3d.isensee2017 import isensee2017_model_3d
from .unet.unet import unet_model_2d
from .unet.isensee import isensee2017_model
from .discriminator.all_dis_2d import discriminator_image_2d
from .discriminator.all_dis_3d import discriminator_image_3d
from .norm.NormNet import norm_net_model
from ..optimizers import SGD, Adam, RMSprop  # noqa: F401
