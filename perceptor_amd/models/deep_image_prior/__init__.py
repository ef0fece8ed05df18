from .deep_image_prior import DeepImagePrior
