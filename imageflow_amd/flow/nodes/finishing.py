"""Mirrors of flow/nodes/round_corners.rs (RoundImageCorners + RoundImageCornersMut) and flow/nodes/white_balance.rs
(WhiteBalanceSrgbMutDef) on device-resident batches."""
from ...graphics.bitmaps import Bitmap, BitmapCompositing


def round_image_corners(b: Bitmap, mode, radii, background_color):
    """RoundImageCorners::expand (:22-53): EnableTransparency when the colour is not opaque (an unused alpha becomes
    255), then RoundImageCornersMut::mutate (:66-93): BlendWithSelf and the clear.  background_color: Color32."""
    from ...graphics.bitmap_ops import normalize_unused_alpha
    from ...graphics.rounded_corners import clear_around_rounded_corners
    if (background_color >> 24) != 255 and not b.alpha_meaningful:
        normalize_unused_alpha(b)
        b.alpha_meaningful = True
    b.compose = BitmapCompositing.BlendWithSelf
    b.matte = 0
    clear_around_rounded_corners(b, mode, radii, background_color)


def white_balance_histogram_area_threshold_srgb(b: Bitmap, threshold=None):
    """WhiteBalanceSrgbMutDef::mutate (:106-122)."""
    from ...graphics.white_balance import white_balance_srgb
    white_balance_srgb(b, threshold)
