from .resize import resize, resize_backward
from .clamp_with_grad import clamp_with_grad, ClampWithGrad
from .super_resolution import SuperResolution
