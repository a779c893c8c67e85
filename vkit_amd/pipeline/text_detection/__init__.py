from .page_assembler import *  # noqa: F401,F403
from .page_assembler import page_assembler_step_factory  # noqa: F401
from .page_background import (  # noqa: F401
    PageBackgroundStep,
    PageBackgroundStepConfig,
    PageBackgroundStepInput,
    PageBackgroundStepKey,
    PageShapeStepOutput,
    page_background_step_factory,
)
from .page_distortion import (  # noqa: F401
    ElementFlattener,
    PageDistortionStep,
    PageDistortionStepConfig,
    PageDistortionStepInput,
    PageDistortionStepOutput,
    page_distortion_step_factory,
)
from .page_resizing import (  # noqa: F401
    PageResizingStep,
    PageResizingStepConfig,
    PageResizingStepInput,
    PageResizingStepOutput,
    page_resizing_step_factory,
)
from .page_cropping import (  # noqa: F401
    CroppedPage,
    DownsampledLabel,
    PageCroppingStep,
    PageCroppingStepConfig,
    PageCroppingStepInput,
    PageCroppingStepOutput,
    page_cropping_step_factory,
)
from .page_text_line_label import (  # noqa: F401
    PageTextLineLabelStep,
    PageTextLineLabelStepConfig,
    PageTextLineLabelStepInput,
    page_text_line_label_step_factory,
)
from .page_text_region import (  # noqa: F401
    ColumnPacker,
    FlattenedTextRegion,
    PageTextRegionInfo,
    PageTextRegionStep,
    PageTextRegionStepOutput,
    TextRegionFlattener,
    build_background_image_for_stacking,
    calculate_boxed_masks_intersected_ratio,
    calculate_boxed_masks_intersected_ratios,
    envelope_pairs,
    intersected_polygon_ratios,
    polygon_overlap_tables,
    post_rotate_flattened_text_regions,
    resize_flattened_text_regions,
    stack_flattened_text_regions,
)
from .page_text_region_label import (  # noqa: F401
    PageCharRegressionLabel,
    PageCharRegressionLabelTag,
    PageTextRegionLabelStep,
    PageTextRegionLabelStepConfig,
    PageTextRegionLabelStepInput,
    PageTextRegionLabelStepOutput,
    Vector,
    page_text_region_label_step_factory,
)
# (its DownsampledLabel stays in the module: the name above is page_cropping's, as in the reference's package)
from .page_text_region_cropping import (  # noqa: F401
    CroppedPageTextRegion,
    PageTextRegionCroppingStep,
    PageTextRegionCroppingStepConfig,
    PageTextRegionCroppingStepInput,
    PageTextRegionCroppingStepOutput,
    page_text_region_cropping_step_factory,
)
from .page_image import (  # noqa: F401
    PageImageStep,
    PageImageStepConfig,
    PageImageStepInput,
    page_image_step_factory,
)
from .page_barcode import (  # noqa: F401
    PageBarcodePlan,
    PageBarcodeStep,
    PageBarcodeStepConfig,
    PageBarcodeStepInput,
    page_barcode_step_factory,
)
from .page_text_line_bounding_box import (  # noqa: F401
    PageTextLineBoundingBoxStep,
    PageTextLineBoundingBoxStepConfig,
    PageTextLineBoundingBoxStepInput,
    TextLineBoundingBoxPlan,
    page_text_line_bounding_box_step_factory,
)
from .page_non_text_symbol import (  # noqa: F401
    NonTextSymbolColorMode,
    NonTextSymbolPlan,
    PageNonTextSymbolStep,
    PageNonTextSymbolStepConfig,
    PageNonTextSymbolStepInput,
    page_non_text_symbol_step_factory,
)
