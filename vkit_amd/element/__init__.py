from .type import Shapable, ElementSetOperationMode
from .point import Point, PointList, PointTuple
from .box import Box
from .polygon import Polygon
from .soup import PointArray, PolygonSoup
from .mask import Mask, MaskSetItemConfig
from .score_map import ScoreMap, ScoreMapSetItemConfig, quad_u, quad_v
from .image import Image, ImageMode, ImageSetItemConfig, encode_jpeg_images
