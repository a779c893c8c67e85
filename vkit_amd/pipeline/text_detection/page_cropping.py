"""PageCroppingStep: the step after page resizing (reference: vkit/pipeline/text_detection/page_cropping.py:74-290).

The reference draws one crop window per attempt (attempt 0 the centre crop, then random proposals), crops seven planes,
rejects the crop on its text ratio (char-mask pixels in the core / core_size^2) or its active ratio (active-mask pixels /
crop_size^2), and shrinks the five labels of an accepted crop with INTER_AREA.  The windows depend on the generator only,
so here they are drawn up front from a COPY of it, for as many attempts as the step could possibly make; then
  1. one launch counts every candidate window (and the page's nonzero pixels when num_samples is unset) -- k_crop_count;
  2. one download brings the counts back, and the reference's loop runs on them as it runs on its numpy counts;
  3. the attempts the loop made are drawn again from the caller's generator, which ends where the reference leaves it;
  4. one launch crops every plane of every accepted window and shrinks the labels -- k_crop_planes.
A device-resident page stays on the device (two launches, one synchronisation); a host page is uploaded and its crops
come back on the host.
"""
import copy
from typing import List, Optional, Sequence, Tuple

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd import _native
from vkit_amd.element import Box, Image, Mask, ScoreMap
from vkit_amd.mechanism.cropper import CropperState
from ..interface import PipelineStep, PipelineStepFactory
from .page_resizing import PageResizingStepOutput


@attrs.define
class PageCroppingStepConfig:
    core_size: int
    pad_size: int
    num_samples: Optional[int] = None
    num_samples_max: Optional[int] = None
    num_samples_estimation_factor: float = 1.5
    pad_value: int = 0
    drop_cropped_page_with_small_text_ratio: bool = True
    text_ratio_min: float = 0.025
    drop_cropped_page_with_small_active_region: bool = True
    active_region_ratio_min: float = 0.4
    enable_downsample_labeling: bool = True
    downsample_labeling_factor: int = 2


@attrs.define
class PageCroppingStepInput:
    page_resizing_step_output: PageResizingStepOutput


@attrs.define
class DownsampledLabel:
    shape: Tuple[int, int]
    page_char_mask: Mask
    page_seal_impression_char_mask: Mask
    page_char_height_score_map: ScoreMap
    page_text_line_mask: Mask
    page_text_line_height_score_map: ScoreMap
    target_core_box: Box


@attrs.define
class CroppedPage:
    page_image: Image
    page_char_mask: Mask
    page_seal_impression_char_mask: Mask
    page_char_height_score_map: ScoreMap
    page_text_line_mask: Mask
    page_text_line_height_score_map: ScoreMap
    target_core_box: Box
    downsampled_label: Optional[DownsampledLabel]


@attrs.define
class PageCroppingStepOutput:
    cropped_pages: Sequence[CroppedPage]


# the five labels, cropped to the core and shrunk (page_cropping.py:117-139, 154-230)
_LABELS = ('page_char_mask', 'page_seal_impression_char_mask', 'page_char_height_score_map', 'page_text_line_mask',
           'page_text_line_height_score_map')


class PageCroppingStep(PipelineStep[PageCroppingStepConfig, PageCroppingStepInput, PageCroppingStepOutput]):

    def __init__(self, config: PageCroppingStepConfig):
        super().__init__(config)

    def _state(self, shape, rng: Optional[RandomGenerator]):
        """The window of one attempt: the centre crop without a generator, a random proposal with one."""
        config = self.config
        if rng is None:
            return CropperState.create_from_center_point(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                         pad_value=config.pad_value,
                                                         center_point=Box.from_shape(shape).get_center_point())
        return CropperState.create_from_random_proposal(shape=shape, core_size=config.core_size, pad_size=config.pad_size,
                                                        pad_value=config.pad_value, rng=rng)

    def _accepted(self, text_pixels: int, active_pixels: int) -> bool:
        """The reference's two rejections, in its order, on its float64 ratios (page_cropping.py:142-152)."""
        config = self.config
        if config.drop_cropped_page_with_small_text_ratio:
            if int(text_pixels) / config.core_size**2 < config.text_ratio_min:
                return False
        if config.drop_cropped_page_with_small_active_region:
            crop_size = config.core_size + 2 * config.pad_size
            if int(active_pixels) / crop_size**2 < config.active_region_ratio_min:
                return False
        return True

    def _estimate(self, page_area: int):
        config = self.config
        num_samples = max(1, round(page_area / config.core_size**2 * config.num_samples_estimation_factor))
        if config.num_samples_max:
            num_samples = min(num_samples, config.num_samples_max)
        return num_samples

    def _crop(self, elements, arrs, states: List[CropperState]) -> List[CroppedPage]:
        """Every plane of every accepted crop in one launch (k_crop_planes), from the device planes ``arrs`` of the
        ``elements``; the crops of a host page come back on the host."""
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
            jobs.append(dict(src=arrs['page_active_mask'], window=index))
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

        cropped_pages = []
        per_crop = 2 + len(_LABELS)
        for index, state in enumerate(states):
            planes = outs[index * per_crop:(index + 1) * per_crop]
            labels, downs = {}, {}
            for name, (core, down) in zip(_LABELS, planes[2:]):
                element = elements[name]
                if isinstance(element, Mask):
                    labels[name] = Mask(mat=core).to_box_attached(state.target_core_box)
                    downs[name] = Mask(mat=down) if factor else None
                else:
                    labels[name] = ScoreMap(mat=core, is_prob=element.is_prob).to_box_attached(state.target_core_box)
                    downs[name] = ScoreMap(mat=down, is_prob=element.is_prob) if factor else None
            downsampled_label = None
            if factor:
                assert state.target_core_box.height == state.target_core_box.width == config.core_size
                begin = config.pad_size // factor
                end = begin + config.core_size // factor - 1
                downsampled_label = DownsampledLabel(shape=(crop_size // factor, crop_size // factor),
                                                     target_core_box=Box(up=begin, down=end, left=begin, right=end), **downs)
            cropped_pages.append(CroppedPage(page_image=Image(mat=planes[0][0]), target_core_box=state.target_core_box,
                                             downsampled_label=downsampled_label, **labels))
        return cropped_pages

    def sample_cropped_page(self, page_image: Image, page_active_mask: Mask, page_char_mask: Mask,
                            page_seal_impression_char_mask: Mask, page_char_height_score_map: ScoreMap,
                            page_text_line_mask: Mask, page_text_line_height_score_map: ScoreMap, rng: RandomGenerator,
                            force_crop_center: bool = False):
        """One attempt (page_cropping.py:87-241): the cropped page, or None when the crop is rejected."""
        elements = dict(page_image=page_image, page_active_mask=page_active_mask, page_char_mask=page_char_mask,
                        page_seal_impression_char_mask=page_seal_impression_char_mask,
                        page_char_height_score_map=page_char_height_score_map, page_text_line_mask=page_text_line_mask,
                        page_text_line_height_score_map=page_text_line_height_score_map)
        state = self._state(page_image.shape, None if force_crop_center else rng)
        arrs = _device_planes(elements)
        _, text, active = _native.crop_count(None, arrs['page_active_mask'], arrs['page_char_mask'], [state.to_crop_window()],
                                             self.config.core_size, self.config.pad_size)
        if not self._accepted(text[0], active[0]):
            return None
        return self._crop(elements, arrs, [state])[0]

    def run(self, input: PageCroppingStepInput, rng: RandomGenerator):
        config = self.config
        src = input.page_resizing_step_output
        elements = {name: getattr(src, name) for name in ('page_image', 'page_active_mask') + _LABELS}
        page_image = elements['page_image']
        assert page_image.arr.ndim == 3 and page_image.arr.shape[2] == 3, 'a 3-channel page image'
        shape = page_image.shape
        for name, element in elements.items():
            assert element.box is None and element.shape == shape, name

        # every attempt the loop could make: num_samples is at most its estimate from the whole page area
        if config.num_samples is None:
            bound = self._estimate(shape[0] * shape[1])
        else:
            bound = config.num_samples
            if config.num_samples_max:
                bound = min(bound, config.num_samples_max)
        probe = copy.deepcopy(rng)
        states = [self._state(shape, None)] + [self._state(shape, probe) for _ in range(max(3, 2 * bound) - 1)]

        arrs = _device_planes(elements)
        page_area, text, active = _native.crop_count(arrs['page_image'] if config.num_samples is None else None,
                                                     arrs['page_active_mask'], arrs['page_char_mask'],
                                                     [state.to_crop_window() for state in states], config.core_size,
                                                     config.pad_size)
        num_samples = self._estimate(page_area) if config.num_samples is None else config.num_samples
        if config.num_samples is not None and config.num_samples_max:
            num_samples = min(num_samples, config.num_samples_max)

        run_count_max = max(3, 2 * num_samples)
        run_count = 0
        accepted: List[CropperState] = []
        while len(accepted) < num_samples and run_count < run_count_max:
            if run_count > 0:
                # the caller's generator makes the draws of this attempt, as the reference's does
                state = self._state(shape, rng)
                assert state == states[run_count]
            if self._accepted(text[run_count], active[run_count]):
                accepted.append(states[run_count])
            run_count += 1

        return PageCroppingStepOutput(cropped_pages=self._crop(elements, arrs, accepted))


def _device_planes(elements):
    """The planes of the page on one context (host planes uploaded once)."""
    ctx = next((e.arr.ctx for e in elements.values() if e.on_device), None) or _native.default_ctx()
    out = {}
    for name, element in elements.items():
        arr = element.arr
        if not isinstance(arr, _native.DevArray):
            arr = ctx.to_device(arr)
        elif arr.ctx is not ctx:
            arr.ctx.sync()
            arr = _native.device_copy(arr, ctx)
        out[name] = arr
    return out


page_cropping_step_factory = PipelineStepFactory(PageCroppingStep)
