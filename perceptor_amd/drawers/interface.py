from torch import nn


class DrawingInterface(nn.Module):
    """A drawer is called like a function and returns its picture; subclasses provide synthesize / encode / replace_."""

    def forward(self, *args, **kwargs):
        return self.synthesize(*args, **kwargs)

    def synthesize(self, *args, **kwargs):
        raise NotImplementedError

    def encode(self, *args, **kwargs):
        raise NotImplementedError

    def replace_(self, *args, **kwargs):
        raise NotImplementedError
