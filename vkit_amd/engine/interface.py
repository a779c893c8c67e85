"""The engine framework of the reference (vkit/engine/interface.py:88-411) for engines that are drawn from a weighted list:
``EngineExecutorFactory(engine_cls, init_config_cls, run_config_cls).create(init_config)`` and
``EngineExecutorAggregatorFactory([...]).create([{'type': ..., 'weight': ..., 'config': {...}}, ...])`` whose ``run(run_config,
rng)`` draws ONE executor with ``rng_choice(rng, executors, probs)`` -- a draw even for a single engine, as in the reference:
it is part of the generator contract -- and runs it.  Configs are structured by ``vkit_amd.utility.dyn_structure`` (an
instance, a mapping of the fields, a JSON path, None for the defaults)."""
import itertools
from os import PathLike
from typing import Any, Mapping, Optional, Sequence, Tuple, Union

import attrs
from numpy.random import Generator as RandomGenerator

from vkit_amd.utility import dyn_structure, is_path_type, normalize_to_probs, read_json_file, rng_choice


@attrs.define
class NoneTypeEngineInitResource:
    pass


class EngineExecutor:

    def __init__(self, engine, run_config_cls):
        self.engine = engine
        self.run_config_cls = run_config_cls

    def get_run_config_cls(self):
        return self.run_config_cls

    def run(self, run_config: Union[Mapping[str, Any], Any], rng: Optional[RandomGenerator] = None):
        run_config = dyn_structure(run_config, self.run_config_cls)
        return self.engine.run(run_config, rng)


class EngineExecutorFactory:

    def __init__(self, engine_cls, init_config_cls, run_config_cls, init_resource_cls=NoneTypeEngineInitResource):
        self.engine_cls, self.init_config_cls, self.run_config_cls = engine_cls, init_config_cls, run_config_cls
        self.init_resource_cls = init_resource_cls

    def get_type_name(self):
        return self.engine_cls.get_type_name()

    def get_init_config_cls(self):
        return self.init_config_cls

    def get_init_resource_cls(self):
        return self.init_resource_cls

    def create(self, init_config: Optional[Union[Mapping[str, Any], str, PathLike, Any]] = None, init_resource: Optional[Any] = None):
        init_config = dyn_structure(init_config, self.init_config_cls, support_path_type=True, support_none_type=True)
        if self.init_resource_cls is NoneTypeEngineInitResource:
            assert init_resource is None
        else:
            assert init_resource
            init_resource = dyn_structure(init_resource, self.init_resource_cls)
        return EngineExecutor(self.engine_cls(init_config, init_resource), self.run_config_cls)


class EngineExecutorAggregatorSelector:

    def __init__(self, pairs: Sequence[Tuple[EngineExecutor, float]]):
        self.engine_executors = [executor for executor, _ in pairs]
        self.probs = normalize_to_probs([weight for _, weight in pairs])

    def get_run_config_cls(self):
        return self.engine_executors[0].get_run_config_cls()

    def select_engine_executor(self, rng: RandomGenerator):
        return rng_choice(rng, self.engine_executors, probs=self.probs)


def engine_executor_aggregator_default_func_collate(selector: EngineExecutorAggregatorSelector, run_config, rng: RandomGenerator):
    engine_executor = selector.select_engine_executor(rng)
    return engine_executor.run(run_config, rng)


class EngineExecutorAggregator:

    def __init__(self, selector: EngineExecutorAggregatorSelector, func_collate=engine_executor_aggregator_default_func_collate):
        self.selector = selector
        self.func_collate = func_collate

    def get_run_config_cls(self):
        return self.selector.get_run_config_cls()

    def run(self, run_config: Union[Mapping[str, Any], Any], rng: RandomGenerator):
        run_config = dyn_structure(run_config, self.get_run_config_cls())
        return self.func_collate(self.selector, run_config, rng)


def _read_configs(factory_init_configs):
    return read_json_file(factory_init_configs) if is_path_type(factory_init_configs) else factory_init_configs


class EngineExecutorAggregatorFactory:

    def __init__(self, engine_executor_factories: Sequence[EngineExecutorFactory],
                 func_collate=engine_executor_aggregator_default_func_collate):
        self.type_name_to_engine_executor_factory = {factory.get_type_name(): factory for factory in engine_executor_factories}
        self.func_collate = func_collate

    def create(self, factory_init_configs: Union[Sequence[Mapping[str, Any]], str, PathLike],
               init_resources: Optional[Sequence[Any]] = None):
        factory_init_configs = _read_configs(factory_init_configs)
        pairs = []
        for factory_init_config, init_resource in zip(factory_init_configs, init_resources or itertools.repeat(None)):
            type_name = factory_init_config['type']
            if type_name not in self.type_name_to_engine_executor_factory:
                raise KeyError(f'type_name={type_name} not found')
            factory = self.type_name_to_engine_executor_factory[type_name]
            engine_executor = factory.create(factory_init_config.get('config', {}), init_resource)
            # a single engine needs no weight
            weight = 1 if len(factory_init_configs) == 1 else factory_init_config['weight']
            pairs.append((engine_executor, weight))
        return EngineExecutorAggregator(EngineExecutorAggregatorSelector(pairs), func_collate=self.func_collate)

    def create_with_repeated_init_resource(self, factory_init_configs, init_resource):
        factory_init_configs = _read_configs(factory_init_configs)
        return self.create(factory_init_configs, [init_resource] * len(factory_init_configs))

    def create_engine_executor(self, factory_init_config: Mapping[str, Any], init_resource: Optional[Any] = None):
        aggregator = self.create([factory_init_config], [init_resource] if init_resource else None)
        return aggregator.selector.engine_executors[0]
