// Result-set mode (l2_join.h): which rule sets it takes, and its tables.
#include "l2_join.h"
#include "l2_compile.hpp"
#include "l2_tables.h"
#include <map>
#include <set>
#include <string>
#include <vector>

namespace spa {

// returns the reason why the rule set cannot run in join mode (empty = it can).  The entries follow the key index the
// optimizer left behind: a plain key reference gives the entry of the program's meaning (sequence: first term -> second;
// within: the key term -> the other; any: the lexem alone); a reference that the optimizer moved off a frequent event
// (DevKeyRef::pastEvent) gives the JOIN_ALT_* entries of l2_join.h instead.  altPrograms: the programs with such a reference.
std::string buildJoinTables( const FlatTables& ft, std::vector<JoinKey>& keytab, std::vector<JoinRule>& rules, std::vector<uint32_t>& filter, uint32_t& maxRange, uint32_t& delimiter, uint32_t& altPrograms)
{
	std::map<std::pair<uint32_t,uint32_t>,std::vector<JoinRule> > byPair;
	maxRange = 0; delimiter = 0; altPrograms = 0;
	// the key references of every program: how many plain ones per key event, and the moved ones (key event, past event)
	std::vector<std::map<uint32_t,uint32_t> > plainKeys( ft.programs.size());
	std::vector<std::vector<std::pair<uint32_t,uint32_t> > > altKeys( ft.programs.size());
	for (size_t ki=0; ki<ft.keytab.size(); ++ki)
	{
		const DevKeyEntry& ke = ft.keytab[ ki];
		if (!ke.event) continue;
		for (uint32_t r=0; r<ke.listCount; ++r)
		{
			const DevKeyRef& ref = ft.keylist[ ke.listBegin + r];
			if (ref.program >= ft.programs.size()) return "a key reference out of range";
			if (ref.pastEvent) altKeys[ ref.program].push_back( std::make_pair( ke.event, ref.pastEvent));
			else ++plainKeys[ ref.program][ ke.event];
		}
	}
	std::set<uint32_t> listened;
	for (size_t i=0; i<ft.trigdefs.size(); ++i) listened.insert( ft.trigdefs[ i].event);
	for (size_t pi=0; pi<ft.programs.size(); ++pi)
	{
		const DevProgram& p = ft.programs[ pi];
		if (p.event && listened.count( p.event)) return "a program whose result another program listens to";
		if (!p.resultHandle) return "a program without result";
	}
	for (size_t pi=0; pi<ft.programs.size(); ++pi)
	{
		const DevProgram& p = ft.programs[ pi];
		// the two terms and the delimiter of the program.  The plain entries follow the program's meaning -- sequence: first
		// term -> second; within: the key term -> the other; any: each term alone -- one per plain key reference (a program
		// with two equal terms counts twice there, and twice here); a moved reference gives its JOIN_ALT_* entries.
		const DevTrigDef* term[ 2] = {0, 0}; const DevTrigDef* del = 0;
		unsigned nterm = 0;
		for (uint32_t t=0; t<p.trigCount; ++t)
		{
			const DevTrigDef& td = ft.trigdefs[ p.trigBegin + t];
			if ((td.flags & 0xF) == SIG_DEL) { if (del) return "a program with two delimiters"; del = &td; }
			else { if (nterm == 2) return "a program with more than two terms"; term[ nterm++] = &td; }
		}
		if (nterm != 2) return "a program that has not two terms";
		if (term[ 0]->variable > 255 || term[ 1]->variable > 255) return "a variable id beyond 255";
		const uint32_t sigtype = term[ 0]->flags & 0xF;
		if ((term[ 1]->flags & 0xF) != sigtype) return "a program with mixed signals";
		JoinRule r; r.range = p.positionRange; r.resultHandle = p.resultHandle; r.formatHandle = p.formatHandle; r.flags = 0;
		if (del)
		{
			if (delimiter && delimiter != del->event) return "more than one delimiter event";
			delimiter = del->event; r.flags |= JOIN_STRUCT;
			if (term[ 0]->event == delimiter || term[ 1]->event == delimiter) return "the delimiter as a term";
		}
		if (r.range > maxRange) maxRange = r.range;
		if (!altKeys[ pi].empty()) ++altPrograms;
		if (sigtype == SIG_ANY)
		{
			if (p.initcount != 1 || del) return "an `any` program with a cardinality or a delimiter";
			if (!altKeys[ pi].empty()) return "an `any` program with a moved key";
			// (two equal terms: both triggers of both instances take the lexem, term[0] in table order first -- listed last)
			const bool same = term[ 0]->event == term[ 1]->event;
			for (int t=0; t<2; ++t)
			{
				JoinRule rt = r; rt.flags |= same ? ((term[ 1]->variable << 16) | (term[ 0]->variable << 8)) : (term[ t]->variable << 16);
				byPair[ std::make_pair( (uint32_t)JOIN_SELF, term[ t]->event)].push_back( rt);
			}
		}
		else if (sigtype == SIG_SEQUENCE)
		{
			if (p.initcount != 2 || p.initsigval != 2) return "a sequence with a cardinality";
			const int first = term[ 0]->sigval == 2 ? 0 : 1;
			if (term[ first]->sigval != 2 || term[ 1-first]->sigval != 1) return "a sequence with unexpected signal values";
			r.flags |= (term[ first]->variable << 8) | (term[ 1-first]->variable << 16);
			const std::pair<uint32_t,uint32_t> pair( term[ first]->event, term[ 1-first]->event);
			if (plainKeys[ pi].count( term[ first]->event)) byPair[ pair].push_back( r);
			for (size_t a=0; a<altKeys[ pi].size(); ++a)
			{
				if (altKeys[ pi][ a] != std::make_pair( pair.second, pair.first)) return "a sequence moved onto an unexpected key";
				JoinRule ra = r; ra.flags |= JOIN_ALT_SEQ;
				byPair[ pair].push_back( ra);
			}
		}
		else if (sigtype == SIG_WITHIN)
		{
			if (p.initcount != 2) return "a within with a cardinality";
			// (two equal terms: the key lexem is taken by the trigger installed first, term[0] in table order, in both instances)
			const bool same = term[ 0]->event == term[ 1]->event;
			for (int t=0; t<2; ++t)
			{
				const int a = same ? 0 : t;
				std::map<uint32_t,uint32_t>::const_iterator pk = plainKeys[ pi].find( term[ t]->event);
				if (pk == plainKeys[ pi].end() || pk->second < (same ? (uint32_t)t+1 : 1u)) continue;
				JoinRule rt = r; rt.flags |= (term[ a]->variable << 8) | (term[ 1-a]->variable << 16);
				byPair[ std::make_pair( term[ t]->event, term[ 1-t]->event)].push_back( rt);
			}
			// moved onto key term k from its other term p: the replay of the latest p completed by k, and the instance of a
			// k without a replay that waits for a later p
			for (size_t a=0; a<altKeys[ pi].size(); ++a)
			{
				const int k = term[ 0]->event == altKeys[ pi][ a].first ? 0 : 1;
				if (same || term[ k]->event != altKeys[ pi][ a].first || term[ 1-k]->event != altKeys[ pi][ a].second) return "a within moved onto an unexpected key";
				JoinRule rr = r; rr.flags |= JOIN_ALT_REPLAY | (term[ 1-k]->variable << 8) | (term[ k]->variable << 16);
				byPair[ std::make_pair( term[ 1-k]->event, term[ k]->event)].push_back( rr);
				JoinRule rl = r; rl.flags |= JOIN_ALT_LINGER | (term[ k]->variable << 8) | (term[ 1-k]->variable << 16);
				byPair[ std::make_pair( term[ k]->event, term[ 1-k]->event)].push_back( rl);
			}
		}
		else return "a program that is neither sequence, within nor any";
	}
	if (byPair.empty()) return "no program";
	size_t size = 1;
	while (size < byPair.size()*2+1) size <<= 1;
	JoinKey none; none.first = 0; none.second = 0; none.begin = 0; none.count = 0;
	keytab.assign( size, none); rules.clear();
	filter.assign( JOIN_FILTER_WORDS, 0);
	for (std::map<std::pair<uint32_t,uint32_t>,std::vector<JoinRule> >::const_iterator it=byPair.begin(); it!=byPair.end(); ++it)
	{
		JoinKey k; k.first = it->first.first; k.second = it->first.second; k.begin = (uint32_t)rules.size(); k.count = (uint32_t)it->second.size();
		rules.insert( rules.end(), it->second.begin(), it->second.end());
		size_t slot = joinHash( k.first, k.second) & (size-1);
		while (keytab[ slot].first) slot = (slot+1) & (size-1);
		keytab[ slot] = k;
		const uint32_t bit = (joinHash( k.first, k.second) >> 8) % (JOIN_FILTER_WORDS*32u);
		filter[ bit >> 5] |= 1u << (bit & 31u);
	}
	return std::string();
}

} // namespace
