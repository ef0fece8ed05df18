"""Input geometry of the published MonsterDiffusion networks: 48 x 48 RGB sprites, nine non-leaky augmentation flags."""
INPUT_CHANNELS, INPUT_HEIGHT, INPUT_WIDTH = 3, 48, 48
INPUT_SIZE = (INPUT_WIDTH, INPUT_HEIGHT)
INPUT_SHAPE = (INPUT_CHANNELS, INPUT_HEIGHT, INPUT_WIDTH)
N_AUGMENTATIONS = 9
