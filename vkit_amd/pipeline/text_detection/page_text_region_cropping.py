"""PageTextRegionCroppingStep: a labelled text-region page cut into training samples (reference:
vkit/pipeline/text_detection/page_text_region_cropping.py).

Per attempt the reference draws one crop window (on a rotated page: a proposal on the shape before the rotation, whose centre
is rotated onto the page), asks two shapely STRtrees which centroid and which deviate label points the window's
original_core_box intersects, drops the deviate labels of chars whose centroid label fell outside, rejects the attempt when too
few labels are left, and otherwise shifts the labels, crops five planes and shrinks four of them with INTER_AREA.  The windows
depend on the generator only, so here they are drawn up front from a COPY of it, for as many attempts as the loop could make;
then
  1. one launch selects the labels of every candidate window -- k_region_crop_select (csrc/region_crop.hip);
  2. the step's only synchronisation brings the counts back, and the reference's loop runs on them;
  3. the attempts the loop made are drawn again from the caller's generator, which ends where the reference leaves it;
  4. one launch crops every plane of every accepted window and shrinks the labels -- k_crop_planes (csrc/crop.hip);
  5. the kept labels of the accepted windows are shifted and downsampled on the host, centroid labels first, in index order.
A device-resident page stays on the device (two launches, one synchronisation); a host page is uploaded and its crops come
back on the host.

Semantics.  ``Box.to_shapely_polygon().intersects(Point)`` is true for a point on the box's edge, so a label is inside the
core when ``left <= x <= right and up <= y <= down``: closed bounds.  shapely is installed neither where this project is built
nor where it runs, so this boundary is restated from shapely's definition, not pinned against shapely itself (DESIGN.md section 2,
as the cv2 members are).
"""
import copy
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, Image, Mask, ScoreMap
from vkit_amd.mechanism.cropper import CropperState
from vkit_amd.mechanism.distortion import rotate
from ..interface import PipelineStep, PipelineStepFactory
from .page_cropping import PageCroppingStepOutput, _device_planes
from .page_text_region import PageTextRegionStepOutput
from .page_text_region_label import (
    PageCharRegressionLabel,
    PageCharRegressionLabelTag,
    PageTextRegionLabelStepOutput,
)


@attrs.define
class PageTextRegionCroppingStepConfig:
    core_size: int
    pad_size: int
    num_samples_factor_relative_to_num_cropped_pages: float = 1.0
    num_centroid_points_min: int = 10
    num_deviate_points_min: int = 10
    pad_value: int = 0
    enable_downsample_labeling: bool = True
    downsample_labeling_factor: int = 2


@attrs.define
class PageTextRegionCroppingStepInput:
    page_cropping_step_output: PageCroppingStepOutput
    page_text_region_step_output: PageTextRegionStepOutput
    page_text_region_label_step_output: PageTextRegionLabelStepOutput


@attrs.define
class DownsampledLabel:
    shape: Tuple[int, int]
    page_char_mask: Mask
    page_char_height_score_map: ScoreMap
    page_char_gaussian_score_map: ScoreMap
    page_char_regression_labels: Sequence[PageCharRegressionLabel]
    page_char_bounding_box_mask: Mask
    target_core_box: Box


@attrs.define
class CroppedPageTextRegion:
    page_image: Image
    page_char_mask: Mask
    page_char_height_score_map: ScoreMap
    page_char_gaussian_score_map: ScoreMap
    page_char_regression_labels: Sequence[PageCharRegressionLabel]
    page_char_bounding_box_mask: Mask
    target_core_box: Box
    downsampled_label: Optional[DownsampledLabel]


@attrs.define
class PageTextRegionCroppingStepOutput:
    cropped_page_text_regions: Sequence[CroppedPageTextRegion]


# the four labels, cropped to the core and shrunk (page_text_region_cropping.py:211-286)
_LABELS = ('page_char_mask', 'page_char_height_score_map', 'page_char_gaussian_score_map', 'page_char_bounding_box_mask')


def _score_map(arr, is_prob: bool, box: Optional[Box] = None) -> ScoreMap:
    """The ScoreMap of a crop.  The range scan of a probability map would download a device plane, so its range is proven
    instead: the page's map passed that scan when it was made, a crop holds its values and the float32 fill 0, and the shrunk
    plane is clipped to [0, 1] by the kernel (``clip``).  A host plane is scanned as usual."""
    if not is_prob or isinstance(arr, np.ndarray):
        return ScoreMap(mat=arr, box=box, is_prob=is_prob)
    score_map = ScoreMap(mat=arr, box=box, is_prob=False)
    object.__setattr__(score_map, 'is_prob', True)
    return score_map


def label_table(labels: Sequence[PageCharRegressionLabel]) -> np.ndarray:
    """int32 (n, 3) (x, y, char_idx) of the labels' integer points, the points the reference builds its tree from (:98-103)."""
    for label in labels:
        assert not label.is_downsampled
    return np.array([(label.downsampled_label_point_x, label.downsampled_label_point_y, label.char_idx) for label in labels],
                    dtype=np.int32).reshape(-1, 3)


def core_box_table(states: Sequence[CropperState]) -> np.ndarray:
    """int32 (n, 4) (up, down, left, right) of the windows' original_core_box."""
    return np.array([(s.original_core_box.up, s.original_core_box.down, s.original_core_box.left, s.original_core_box.right)
                     for s in states], dtype=np.int32).reshape(-1, 4)


class PageTextRegionCroppingStep(PipelineStep[PageTextRegionCroppingStepConfig, PageTextRegionCroppingStepInput,
                                              PageTextRegionCroppingStepOutput]):

    def __init__(self, config: PageTextRegionCroppingStepConfig):
        super().__init__(config)

    def _state(self, shape, shape_before_rotate, rotate_angle, rng: RandomGenerator) -> CropperState:
        """The window of one attempt (:123-158)."""
        config = self.config
        if rotate_angle == 0:
            return CropperState.create_from_random_proposal(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                            pad_value=config.pad_value, rng=rng)
        before = CropperState.create_from_random_proposal(shape=shape_before_rotate, core_size=config.core_size,
                                                          pad_size=config.pad_size, pad_value=config.pad_value, rng=rng)
        rotated_result = rotate.distort({'angle': rotate_angle}, shapable_or_shape=shape_before_rotate,
                                        point=before.original_box.get_center_point())
        assert rotated_result.shape == shape
        center_point = rotated_result.point
        assert center_point
        return CropperState.create_from_center_point(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                     pad_value=config.pad_value, center_point=center_point)

    def _accepted(self, counts) -> bool:
        """The reference's rejection (:189-191) on the two counts of a window."""
        return not (int(counts[0]) < self.config.num_centroid_points_min
                    or int(counts[1]) < self.config.num_deviate_points_min)

    def _crop(self, elements, arrs, states: List[CropperState], kept_labels) -> List[CroppedPageTextRegion]:
        """The samples of the accepted windows: every plane in one launch (k_crop_planes) from the device planes ``arrs`` of
        the ``elements``, the crops of a host page back on the host; ``kept_labels`` the (centroid, deviate) labels of each
        window, in index order."""
        if not states:
            return []
        config = self.config
        factor = config.downsample_labeling_factor if config.enable_downsample_labeling else 0
        crop_size = config.core_size + 2 * config.pad_size
        if factor:
            assert crop_size % factor == 0
            assert config.pad_size % factor == 0
            assert config.core_size % factor == 0
        jobs = []
        for index in range(len(states)):
            jobs.append(dict(src=arrs['page_image'], window=index, fill=config.pad_value))
            for name in _LABELS:
                element = elements[name]
                is_mask = isinstance(element, Mask)
                jobs.append(dict(src=arrs[name], window=index, core_only=True, down=bool(factor), is_mask=is_mask,
                                 clip=(not is_mask) and element.is_prob))
        shape = elements['page_image'].shape
        outs = _native.crop_planes(jobs, [state.to_crop_window() for state in states], shape, config.core_size, config.pad_size,
                                   factor)
        if not elements['page_image'].on_device:
            outs = [tuple(None if a is None else a.host() for a in pair) for pair in outs]

        samples = []
        per_crop = 1 + len(_LABELS)
        for index, state in enumerate(states):
            planes = outs[index * per_crop:(index + 1) * per_crop]
            labels, downs = {}, {}
            for name, (core, down) in zip(_LABELS, planes[1:]):
                element = elements[name]
                if isinstance(element, Mask):
                    labels[name] = Mask(mat=core).to_box_attached(state.target_core_box)
                    downs[name] = Mask(mat=down) if factor else None
                else:
                    labels[name] = _score_map(core, element.is_prob, state.target_core_box)
                    downs[name] = _score_map(down, element.is_prob) if factor else None

            # shift the labels (:193-207): centroid labels, then deviate labels
            offset_y = state.target_box.up - state.original_box.up
            offset_x = state.target_box.left - state.original_box.left
            shifted = [label.to_shifted_page_char_regression_label(offset_y=offset_y, offset_x=offset_x)
                       for group in kept_labels[index] for label in group]

            downsampled_label = None
            if factor:
                assert state.target_core_box.height == state.target_core_box.width == config.core_size
                begin = config.pad_size // factor
                end = begin + config.core_size // factor - 1
                downsampled_label = DownsampledLabel(
                    shape=(crop_size // factor, crop_size // factor),
                    page_char_regression_labels=[label.to_downsampled_page_char_regression_label(factor) for label in shifted],
                    target_core_box=Box(up=begin, down=end, left=begin, right=end), **downs)
            samples.append(CroppedPageTextRegion(page_image=Image(mat=planes[0][0]), page_char_regression_labels=shifted,
                                                 target_core_box=state.target_core_box, downsampled_label=downsampled_label,
                                                 **labels))
        return samples

    def sample_cropped_page_text_regions(
        self,
        page_image: Image,
        shape_before_rotate: Tuple[int, int],
        rotate_angle: int,
        page_char_mask: Mask,
        page_char_height_score_map: ScoreMap,
        page_char_gaussian_score_map: ScoreMap,
        page_char_bounding_box_mask: Mask,
        centroid_page_char_regression_labels: Sequence[PageCharRegressionLabel],
        deviate_page_char_regression_labels: Sequence[PageCharRegressionLabel],
        rng: RandomGenerator,
    ):
        """One attempt (:108-313; the two trees are replaced by their label sequences): the sample, or None when rejected."""
        elements = dict(page_image=page_image, page_char_mask=page_char_mask,
                        page_char_height_score_map=page_char_height_score_map,
                        page_char_gaussian_score_map=page_char_gaussian_score_map,
                        page_char_bounding_box_mask=page_char_bounding_box_mask)
        state = self._state(page_image.shape, shape_before_rotate, rotate_angle, rng)
        arrs = _device_planes(elements)
        counts, centroid_rows, deviate_rows = _native.region_crop_select(
            core_box_table([state]), label_table(centroid_page_char_regression_labels),
            label_table(deviate_page_char_regression_labels), ctx=arrs['page_image'].ctx)
        if not self._accepted(counts[0]):
            return None
        kept = ([centroid_page_char_regression_labels[k] for k in centroid_rows[0].tolist()],
                [deviate_page_char_regression_labels[k] for k in deviate_rows[0].tolist()])
        return self._crop(elements, arrs, [state], [kept])[0]

    def run(self, input: PageTextRegionCroppingStepInput, rng: RandomGenerator):
        config = self.config
        num_cropped_pages = len(input.page_cropping_step_output.cropped_pages)
        region = input.page_text_region_step_output
        src = input.page_text_region_label_step_output
        elements = dict(page_image=region.page_image, **{name: getattr(src, name) for name in _LABELS})
        shape = region.page_image.shape
        for name, element in elements.items():
            assert element.box is None and element.shape == shape, name

        # 1. the labels by tag, as the reference splits them before it builds its trees (:334-348)
        labels = src.page_char_regression_labels
        centroid_labels = [label for label in labels if label.tag == PageCharRegressionLabelTag.CENTROID]
        deviate_labels = [label for label in labels if label.tag == PageCharRegressionLabelTag.DEVIATE]
        centroid_table, deviate_table = label_table(centroid_labels), label_table(deviate_labels)

        # 2. every attempt the loop could make, drawn from a copy of the generator
        num_samples = round(config.num_samples_factor_relative_to_num_cropped_pages * num_cropped_pages)
        run_count_max = max(3, 2 * num_samples)
        if num_samples <= 0:
            return PageTextRegionCroppingStepOutput(cropped_page_text_regions=[])
        probe = copy.deepcopy(rng)
        states = [self._state(shape, region.shape_before_rotate, region.rotate_angle, probe) for _ in range(run_count_max)]

        # 3. the selection of every candidate (the step's only synchronisation)
        arrs = _device_planes(elements)
        counts, centroid_rows, deviate_rows = _native.region_crop_select(core_box_table(states), centroid_table, deviate_table,
                                                                         ctx=arrs['page_image'].ctx)

        # 4. the reference's loop (:354-376) on the counts
        run_count = 0
        accepted: List[int] = []
        while len(accepted) < num_samples and run_count < run_count_max:
            # the caller's generator makes the draws of this attempt, as the reference's does
            state = self._state(shape, region.shape_before_rotate, region.rotate_angle, rng)
            assert state == states[run_count]
            if self._accepted(counts[run_count]):
                accepted.append(run_count)
            run_count += 1

        # 5, 6. the planes and the labels of the accepted windows
        kept = [([centroid_labels[k] for k in centroid_rows[index].tolist()],
                 [deviate_labels[k] for k in deviate_rows[index].tolist()]) for index in accepted]
        return PageTextRegionCroppingStepOutput(
            cropped_page_text_regions=self._crop(elements, arrs, [states[index] for index in accepted], kept))


page_text_region_cropping_step_factory = PipelineStepFactory(PageTextRegionCroppingStep)
