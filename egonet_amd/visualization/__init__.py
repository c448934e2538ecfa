"""Drawing predictions: primitive lists on the host (a few hundred rows), rasterised by csrc/overlay.hip; the
training debug pictures (``debug``: csrc/debug_pictures.hip composes, the same rasteriser marks)."""
from .overlay import (CUBOID_EDGES, OverlayRenderer, build_bev_primitives, build_primitives,  # noqa: F401
                      parse_color)
