"""The walk cases of tests/test_walk_pin_gpu.py: case -> the walk keys (plan_census.walk_of) that ONLY this case makes among the pinned
cases of its model and dtype -- what it is in the table for.  A case is (model, c, H, W, dtype, n, variant of plan_census.VARIANTS,
HRN_HALF_STAGES or None for the variant's own).  The table is a minimal cover, found by a greedy search over calls of 3 to 256 crops at
heights up to 224: tests/test_plan_census.py asserts that it covers every walk a production call makes, that every case is needed, and
that each case's plan has the walks named here; the GPU test asserts them again on the live handle.  The fp16 cases repeat their bf16
twins (plan_census.FP16_TWINS)."""
WALK_FOR = {
    ('HRNet', 48, 32, 32, 'bf16', 8, 'long_unfused', 256): [
        ('walk', 1, 48, 3, 0, 512, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 48, 32, 160, 'bf16', 3, 'long', 256): [
        ('slide', 41),
    ],
    ('HRNet', 48, 32, 192, 'bf16', 3, 'long', 256): [
        ('slide', 49),
    ],
    ('HRNet', 48, 32, 192, 'bf16', 3, 'long_unfused', 256): [
        ('walk', 1, 48, 3, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 48, 32, 224, 'bf16', 3, 'long', 256): [
        ('slide', 57),
    ],
    ('HRNet', 48, 32, 224, 'fp16', 3, 'long', 256): [
        ('slide', 57),
    ],
    ('HRNet', 48, 32, 256, 'bf16', 3, 'long', 256): [
        ('slide', 65),
    ],
    ('HRNet', 48, 32, 288, 'bf16', 3, 'long', 256): [
        ('slide', 73),
    ],
    ('HRNet', 48, 32, 288, 'fp16', 3, 'long', 256): [
        ('slide', 73),
    ],
    ('HRNet', 48, 64, 64, 'bf16', 8, 'long_unfused', 256): [
        ('walk', 1, 48, 3, 0, 512, 'plain', 2, 'back', 'none'),
        ('walk', 1, 48, 3, 0, 512, 'plain', 2, 'fwd', 'none'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 1, 'back', 'full'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 1, 'fwd', 'full'),
    ],
    ('HRNet', 48, 96, 32, 'bf16', 12, 'default', None): [
        ('stem_run', 2),
    ],
    ('HRNet', 48, 64, 352, 'bf16', 3, 'long', 1024): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 3, 'fwd', 'ragged'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 2, 'back', 'ragged'),
    ],
    ('HRNet', 48, 64, 352, 'fp16', 3, 'long', 1024): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 3, 'fwd', 'ragged'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 2, 'back', 'ragged'),
    ],
    ('HRNet', 48, 32, 704, 'bf16', 3, 'long', 1024): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 2, 'back', 'ragged'),
    ],
    ('HRNet', 48, 32, 704, 'fp16', 3, 'long', 1024): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 2, 'back', 'ragged'),
    ],
    ('HRNet', 48, 32, 864, 'bf16', 5, 'long', 1536): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 3, 'back', 'ragged'),
    ],
    ('HRNet', 48, 96, 480, 'bf16', 16, 'staged', None): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 3, 32, 6, 0, 512, 'plain', 2, 'back', 'full'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 3, 'back', 'ragged'),
    ],
    ('HRNet', 48, 32, 32, 'bf16', 256, 'staged_unfused', 1024): [
        ('walk', 1, 48, 3, 0, 512, 'plain', 3, 'back', 'none'),
        ('walk', 1, 48, 3, 0, 512, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 512, 'plain', 3, 'fwd', 'none'),
    ],
    ('HRNet', 48, 96, 32, 'bf16', 128, 'default', None): [
        ('walk', 1, 32, 4, 0, 128, 'small', 1, 'back', 'full'),
        ('walk', 1, 48, 3, 0, 128, 'small', 1, 'back', 'full'),
        ('walk', 1, 48, 3, 0, 128, 'small', 1, 'fwd', 'full'),
        ('walk', 1, 48, 3, 0, 512, 'plain', 1, 'back', 'ragged'),
        ('walk', 1, 48, 3, 0, 512, 'plain', 1, 'fwd', 'none'),
    ],
    ('HRNet', 48, 160, 32, 'bf16', 128, 'staged', 3072): [
        ('walk', 1, 32, 3, 0, 512, 'plain', 3, 'back', 'none'),
        ('walk', 1, 32, 3, 0, 512, 'plain', 3, 'back', 'ragged'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 3, 'back', 'full'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 3, 'back', 'none'),
        ('walk', 3, 32, 6, 1, 512, 'plain', 3, 'fwd', 'none'),
    ],
    ('HRNet', 48, 64, 96, 'bf16', 128, 'staged', 1024): [
        ('slide', 25),
        ('walk', 3, 32, 6, 1, 512, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 48, 64, 128, 'bf16', 128, 'staged_small', 256): [
        ('slide', 33),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'back', 'full'),
        ('walk', 3, 32, 6, 1, 128, 'small', 1, 'back', 'full'),
        ('walk', 3, 32, 6, 1, 128, 'small', 1, 'fwd', 'full'),
    ],
    ('HRNet', 48, 32, 320, 'bf16', 128, 'staged', 1024): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 320, 'bf16', 128, 'staged', 1536): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 736, 'bf16', 128, 'forced', None): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 1, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 736, 'bf16', 128, 'staged', 1024): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 736, 'bf16', 128, 'staged', 1536): [
        ('walk', 3, 32, 6, 0, 384, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 384, 'bf16', 256, 'default', None): [
        ('walk', 1, 32, 3, 0, 384, 'plain', 1, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 1, 'back', 'full'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 1, 'back', 'full'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 1, 'fwd', 'full'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 2, 'back', 'full'),
        ('walk', 1, 48, 3, 0, 384, 'plain', 2, 'fwd', 'full'),
    ],
    ('HRNet', 48, 32, 608, 'bf16', 256, 'staged_small', None): [
        ('direct', 3, 2, 6, 4),
        ('walk', 3, 32, 6, 0, 512, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 3, 'long_small', None): [
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'ragged'),
        ('walk', 1, 16, 3, 0, 128, 'small', 2, 'back', 'ragged'),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 8, 'forced', None): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 1, 'fwd', 'none'),
    ],
    ('HRNet', 48, 96, 32, 'fp32', 5, 'long', 512): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'fwd', 'none'),
    ],
    ('HRNet', 48, 32, 320, 'fp32', 3, 'long', 512): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 16, 3, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 16, 3, 0, 384, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 48, 32, 416, 'fp32', 3, 'long', 768): [
        ('walk', 1, 16, 3, 0, 512, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 48, 160, 480, 'fp32', 16, 'staged', None): [
        ('walk', 1, 16, 3, 0, 512, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 48, 96, 864, 'fp32', 16, 'default', None): [
        ('direct', 3, 1, 3, 4),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 256, 'staged', 768): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 256, 'staged_small', 384): [
        ('walk', 1, 16, 2, 0, 128, 'small', 1, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 1, 'fwd', 'full'),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 256, 'staged_small', 512): [
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'none'),
    ],
    ('HRNet', 48, 32, 32, 'fp32', 256, 'staged', 3072): [
        ('walk', 1, 16, 3, 0, 512, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 320, 'fp32', 128, 'staged', 384): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 1, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 352, 'fp32', 128, 'staged', 1024): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'back', 'full'),
        ('walk', 1, 16, 3, 0, 384, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 48, 32, 512, 'fp32', 128, 'staged', 512): [
        ('direct', 3, 2, 4, 2),
    ],
    ('HRNet', 48, 32, 512, 'fp32', 256, 'default', None): [
        ('direct', 3, 2, 4, 4),
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'fwd', 'full'),
    ],
    ('HRNet', 32, 64, 32, 'bf16', 3, 'long_small', None): [
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'back', 'ragged'),
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 32, 224, 'bf16', 3, 'long', 128): [
        ('walk', 1, 32, 2, 0, 512, 'plain', 2, 'fwd', 'none'),
        ('walk', 1, 32, 2, 0, 512, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 32, 320, 'bf16', 3, 'long', 1024): [
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 32, 320, 'bf16', 3, 'long', 128): [
        ('walk', 1, 32, 2, 0, 384, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 96, 32, 'bf16', 12, 'default', None): [
        ('stem_run', 2),
    ],
    ('HRNet', 32, 32, 32, 'bf16', 128, 'staged_small', 256): [
        ('walk', 1, 32, 2, 0, 128, 'small', 1, 'fwd', 'full'),
    ],
    ('HRNet', 32, 32, 32, 'bf16', 128, 'staged', 192): [
        ('walk', 1, 32, 2, 0, 512, 'plain', 3, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 96, 32, 'bf16', 256, 'staged', 1024): [
        ('chain', 'conv2', 2, 'back'),
        ('chain', 'conv2', 2, 'fwd'),
        ('chain', 'conv2_last', 2, 'back'),
        ('chain', 'shortcut', 2, 'fwd'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'fwd', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 3, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 3, 'back', 'none'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 3, 'fwd', 'none'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 3, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 32, 320, 'bf16', 128, 'staged_small', 256): [
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'back', 'full'),
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'back', 'none'),
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'fwd', 'full'),
        ('walk', 1, 32, 2, 0, 384, 'plain', 3, 'fwd', 'none'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 32, 32, 384, 'bf16', 128, 'staged', 128): [
        ('walk', 1, 32, 2, 0, 384, 'plain', 1, 'fwd', 'full'),
    ],
    ('HRNet', 32, 32, 384, 'bf16', 256, 'staged', 128): [
        ('walk', 1, 32, 2, 0, 384, 'plain', 2, 'fwd', 'full'),
    ],
    ('HRNet', 32, 32, 1184, 'bf16', 128, 'default', None): [
        ('direct', 3, 2, 4, 4),
    ],
    ('HRNet', 32, 64, 32, 'fp32', 3, 'long_small', None): [
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'ragged'),
        ('walk', 1, 16, 2, 0, 128, 'small', 3, 'back', 'ragged'),
    ],
    ('HRNet', 32, 32, 416, 'fp32', 3, 'long', 512): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'fwd', 'ragged'),
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'fwd', 'ragged'),
    ],
    ('HRNet', 32, 32, 32, 'fp32', 256, 'staged_small', 512): [
        ('walk', 1, 16, 2, 0, 128, 'small', 1, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 1, 'fwd', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'none'),
        ('walk', 1, 16, 2, 0, 128, 'small', 3, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 3, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 128, 'small', 3, 'fwd', 'none'),
    ],
    ('HRNet', 32, 32, 32, 'fp32', 256, 'staged', 3072): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'back', 'full'),
    ],
    ('HRNet', 32, 64, 32, 'fp32', 256, 'staged', 3072): [
        ('direct', 3, 2, 2, 2),
        ('walk', 1, 16, 2, 0, 512, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 32, 32, 320, 'fp32', 128, 'staged', 512): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'back', 'full'),
    ],
    ('HRNet', 32, 32, 320, 'fp32', 256, 'default', None): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'fwd', 'full'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 1, 'back', 'full'),
    ],
    ('HRNet', 32, 32, 608, 'fp32', 256, 'default', None): [
        ('direct', 3, 2, 4, 4),
    ],
    ('PoseResNet', 50, 32, 32, 'bf16', 3, 'long_small', None): [
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'back', 'ragged'),
    ],
    ('PoseResNet', 50, 32, 32, 'bf16', 256, 'staged', 1024): [
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'fwd', 'full'),
    ],
    ('PoseResNet', 50, 96, 64, 'bf16', 128, 'staged', 1024): [
        ('direct', 2, 1, 4, 2),
        ('walk', 1, 32, 4, 0, 384, 'plain', 1, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 1, 'fwd', 'full'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'back', 'ragged'),
        ('walk', 1, 32, 4, 0, 384, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('PoseResNet', 50, 32, 128, 'bf16', 256, 'staged_small', 512): [
        ('chain', 'conv2', 3, 'back'),
        ('chain', 'conv2_last', 3, 'fwd'),
        ('chain', 'shortcut', 3, 'fwd'),
        ('walk', 1, 32, 4, 0, 128, 'small', 1, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 128, 'small', 1, 'fwd', 'full'),
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'back', 'full'),
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'back', 'none'),
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'fwd', 'full'),
        ('walk', 1, 32, 4, 0, 128, 'small', 2, 'fwd', 'none'),
    ],
    ('PoseResNet', 50, 32, 32, 'fp32', 3, 'long_small', None): [
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'ragged'),
    ],
    ('PoseResNet', 50, 32, 320, 'fp32', 3, 'long', 512): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'back', 'ragged'),
    ],
    ('PoseResNet', 50, 32, 512, 'fp32', 3, 'long', 1024): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'back', 'ragged'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'fwd', 'ragged'),
    ],
    ('PoseResNet', 50, 32, 32, 'fp32', 256, 'staged_small', 512): [
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'full'),
        ('walk', 1, 16, 2, 0, 128, 'small', 2, 'fwd', 'none'),
    ],
    ('PoseResNet', 50, 32, 32, 'fp32', 256, 'staged', None): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'back', 'full'),
    ],
    ('PoseResNet', 50, 64, 32, 'fp32', 256, 'staged', 1024): [
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'back', 'none'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 2, 'fwd', 'none'),
    ],
    ('PoseResNet', 50, 32, 320, 'fp32', 128, 'default', None): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 1, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 384, 'plain', 1, 'fwd', 'full'),
    ],
    ('PoseResNet', 50, 32, 352, 'fp32', 128, 'staged', None): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 3, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 512, 'plain', 3, 'back', 'full'),
    ],
    ('PoseResNet', 50, 32, 320, 'fp32', 256, 'staged', 512): [
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'back', 'full'),
        ('walk', 1, 16, 2, 0, 384, 'plain', 2, 'fwd', 'full'),
    ],
    # the generic kernel's mr = 2 on the stride-2 groups that really launch (a slab launch too small for the slab kernel falls back to them)
    ('HRNet', 48, 32, 192, 'bf16', 128, 'default', None): [
        ('direct', 3, 2, 3, 2),
    ],
    ('HRNet', 32, 32, 256, 'bf16', 96, 'default', None): [
        ('direct', 3, 2, 2, 2),
    ],
    ('HRNet', 32, 32, 1184, 'bf16', 64, 'default', None): [
        ('direct', 3, 2, 4, 2),
    ],
}
